"""cp_stark_prove_batch at the drop-in boundary, without a GPU: the header declares it, the built library exports it, the ctypes
mirror and the generated Rust FFI list it, and the argument refusals that need no context (n_traces out of [1, 64], NULL arrays:
checked before the context is looked at) come back as CP_ERR_INVALID_ARG with a message. The refusals that need a context are in
tests/test_gpu_stark_batch.py."""
import ctypes
import os
import re

import cityprover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1   # CP_ERR_INVALID_ARG


def test_header_library_mirror_and_ffi_list_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cityprover.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cp_stark_prove_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/cityprover.h does not declare cp_stark_prove_batch"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 12 and params[2] == "size_t n_traces" and params[3] == "const uint64_t *const *trace_values"
    assert re.search(r"#define\s+CP_STARK_BATCH_MAX\s+64\b", hdr)
    lib = cityprover.load_library()
    assert hasattr(lib, "cp_stark_prove_batch")
    assert lib.cp_abi_version() == 4          # adding an entry point is additive
    restype, argtypes = cityprover.ABI["cp_stark_prove_batch"]
    assert restype is ctypes.c_int and len(argtypes) == 12
    assert cityprover.STARK_BATCH_MAX == 64 and callable(cityprover.stark_prove_batch)
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    assert "pub fn cp_stark_prove_batch(ctx: *mut CpCtx, desc: *const CpStarkDesc, n_traces: usize, trace_values: *const *const u64," in ffi
    assert "pub const CP_STARK_BATCH_MAX: usize = 64;" in ffi
    assert "ffi::cp_stark_prove_batch(" in open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "lib.rs")).read()


def test_refusals_that_need_no_context():
    lib = cityprover.load_library()
    n = 65
    traces = (ctypes.c_void_p * n)()
    chs = (cityprover.ChallengerState * n)()
    outs, lens = (ctypes.POINTER(ctypes.c_uint8) * n)(), (ctypes.c_size_t * n)()
    sentinel = ctypes.cast(0x5A5A5A50, ctypes.POINTER(ctypes.c_uint8))
    for i in range(n):
        outs[i], lens[i] = sentinel, 7
    before = bytes(chs)

    def call(n_traces, t=traces, c=chs, o=outs, ln=lens):
        return lib.cp_stark_prove_batch(None, None, n_traces, t, 0, None, None, c, None, None, o, ln)

    for bad in (0, 65, 1 << 40):
        assert call(bad) == INVALID_ARG
        assert b"n_traces" in lib.cp_last_error(None) and b"[1, 64]" in lib.cp_last_error(None)
    for kw in (dict(t=None), dict(c=None), dict(o=None), dict(ln=None)):
        assert call(3, **kw) == INVALID_ARG
        assert b"NULL argument" in lib.cp_last_error(None)
    assert call(3) == INVALID_ARG and b"ctx is NULL" in lib.cp_last_error(None)   # in range and complete: only now the context
    # nothing of the caller's was written
    assert bytes(chs) == before
    assert all(ctypes.cast(outs[i], ctypes.c_void_p).value == 0x5A5A5A50 and lens[i] == 7 for i in range(n))
