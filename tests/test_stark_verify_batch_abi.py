"""cp_stark_verify_batch at the drop-in boundary, without a GPU: the header declares it, the built library exports it, the ctypes
mirror and the generated Rust FFI list it, the safe wrapper calls it, and the argument refusals that need no context (NULL arrays,
no proofs, an unknown path form, no description: all checked before the context is looked at) come back as CP_ERR_INVALID_ARG
with a message and write nothing. What needs a description - and so a context - is in tests/test_gpu_stark_verify_batch.py."""
import ctypes
import os
import re

import numpy as np

import cityprover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1   # CP_ERR_INVALID_ARG
PARAMS = ["cp_ctx *ctx", "const cp_stark_desc *desc", "size_t n_proofs", "const uint64_t *publics", "const uint64_t *globals",
          "cp_challenger_state *challengers", "const uint8_t *const *proofs", "const size_t *proof_lens", "size_t chunk_proofs",
          "unsigned path_form", "cp_verify_verdict *verdicts_out"]


def test_header_library_mirror_and_ffi_list_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cityprover.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cp_stark_verify_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/cityprover.h does not declare cp_stark_verify_batch"
    assert [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")] == PARAMS
    for name, v in (("AUTO", 0), ("LANE", 1), ("COOP", 2)):
        assert re.search(r"#define\s+CP_PATHS_%s\s+%du\b" % (name, v), hdr)
    lib = cityprover.load_library()
    assert hasattr(lib, "cp_stark_verify_batch")
    assert lib.cp_abi_version() == 4          # adding an entry point is additive
    restype, argtypes = cityprover.ABI["cp_stark_verify_batch"]
    assert restype is ctypes.c_int and len(argtypes) == len(PARAMS) and argtypes[9] is ctypes.c_uint
    assert (cityprover.PATHS_AUTO, cityprover.PATHS_LANE, cityprover.PATHS_COOP) == (0, 1, 2) and callable(cityprover.stark_verify_batch)
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    assert ("pub fn cp_stark_verify_batch(ctx: *mut CpCtx, desc: *const CpStarkDesc, n_proofs: usize, publics: *const u64, globals: *const u64, "
            "challengers: *mut CpChallengerState, proofs: *const *const u8, proof_lens: *const usize, chunk_proofs: usize, path_form: c_uint, "
            "verdicts_out: *mut CpVerifyVerdict) -> c_int;") in ffi
    assert "pub const CP_PATHS_COOP: c_uint = 2;" in ffi
    assert "ffi::cp_stark_verify_batch(" in open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "lib.rs")).read()


def test_refusals_that_need_no_context():
    lib = cityprover.load_library()
    n = 3
    blobs = [b"\x01" * 64] * n
    ptrs = (ctypes.c_char_p * n)(*blobs)
    lens = (ctypes.c_size_t * n)(*[len(b) for b in blobs])
    chs = (cityprover.ChallengerState * n)()
    verdicts = np.full(n, 0x5A5A5A5A, dtype=cityprover.VERDICT)
    before_ch, before_v = bytes(chs), verdicts.tobytes()
    desc = cityprover.StarkDesc()   # all zero: no constraints program, refused as a description

    def call(n_proofs=n, d=ctypes.byref(desc), c=chs, p=ptrs, ln=lens, form=0, v=verdicts.ctypes.data):
        return lib.cp_stark_verify_batch(None, d, n_proofs, None, None, c, p, ln, 0, form, v)

    for kw in (dict(c=None), dict(p=None), dict(ln=None), dict(v=None)):
        assert call(**kw) == INVALID_ARG
        assert b"NULL argument" in lib.cp_last_error(None)
    assert call(n_proofs=0) == INVALID_ARG and b"no proofs" in lib.cp_last_error(None)
    for form in (3, 255, 2**32 - 1):
        assert call(form=form) == INVALID_ARG and b"path_form" in lib.cp_last_error(None)
    assert call(d=None) == INVALID_ARG and b"desc is NULL" in lib.cp_last_error(None)
    # complete arrays, a known form - and a description that is none: still no word about the context, which is looked at last
    for form in (0, 1, 2):
        assert call(form=form) == INVALID_ARG
        assert b"ctx" not in lib.cp_last_error(None) and lib.cp_last_error(None)
    # nothing of the caller's was written
    assert bytes(chs) == before_ch and verdicts.tobytes() == before_v
