"""The four witness-check entry points at the drop-in boundary, without a GPU: the header declares them, the built library exports
them, the ctypes mirror and the generated Rust FFI list them with the header's parameter lists, the report structures have the
header's layout, and a NULL context or circuit comes back as a status and a message, never a crash. What needs a device is in
tests/test_gpu_check_witness.py and tests/test_gpu_air_check.py."""
import ctypes
import os
import re

import cityprover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1   # CP_ERR_INVALID_ARG
SYMBOLS = {"cp_circuit_check_witness_dev": 8, "cp_circuit_check_witness": 6, "cp_air_check_rows_dev": 9, "cp_stark_check_trace": 9}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cityprover.h")).read(), flags=re.S)


def test_header_library_mirror_and_ffi_list_the_entry_points():
    hdr = header()
    lib = cityprover.load_library()
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    for sym, n_params in SYMBOLS.items():
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, "include/cityprover.h does not declare " + sym
        assert len(m.group(1).split(",")) == n_params, sym
        assert hasattr(lib, sym), sym + " is not exported"
        restype, argtypes = cityprover.ABI[sym]
        assert restype is ctypes.c_int and len(argtypes) == n_params, sym
        assert "pub fn %s(" % sym in ffi, sym + " is missing from the generated Rust FFI"
    assert lib.cp_abi_version() == 4          # adding entry points is additive
    assert re.search(r"#define\s+CP_ABI_VERSION\s+4\b", hdr)
    for f in ("check_witness", "check_witness_batch_dev", "stark_check_trace"):
        assert callable(getattr(cityprover, f))
    assert callable(cityprover.AirProgram.check_rows)


def struct_fields(hdr, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_report_structures_mirror_the_header():
    hdr = header()
    ctype_of = {"uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    for name, mirror, size in (("cp_witness_report", cityprover.WitnessReport, 144), ("cp_air_check_report", cityprover.AirCheckReport, 40)):
        want = [(n, ctype_of[t]) for n, t in struct_fields(hdr, name)]
        assert list(mirror._fields_) == want, name
        assert ctypes.sizeof(mirror) == size, name
    # the order of the fields: counts, then the first gate violation, copy violation, sigma cell, non-canonical cell
    names = [n for n, _ in cityprover.WitnessReport._fields_]
    assert names[:4] == ["n_gate_violations", "n_copy_violations", "n_sigma_undecodable", "n_noncanonical"]
    assert names[4:9] == ["gate_row", "gate_index", "gate_type", "constraint", "constraint_value"]
    assert [n for n, _ in cityprover.AirCheckReport._fields_] == ["n_violations", "row", "sink", "sink_kind", "value"]


def test_null_context_or_circuit_is_a_status_and_a_message():
    lib = cityprover.load_library()
    wr, ar = cityprover.WitnessReport(), cityprover.AirCheckReport()
    one = (ctypes.c_size_t * 1)(0)
    circs = (ctypes.c_void_p * 1)()
    pis = (ctypes.POINTER(ctypes.c_uint64) * 1)()
    assert lib.cp_circuit_check_witness_dev(None, 1, circs, pis, one, None, ctypes.byref(wr), None) == INVALID_ARG
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_circuit_check_witness(None, None, None, 0, ctypes.byref(wr), None) == INVALID_ARG
    assert b"circuit is NULL" in lib.cp_last_error(None)
    assert lib.cp_air_check_rows_dev(None, None, None, 8, None, None, None, ctypes.byref(ar), None) == INVALID_ARG
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_stark_check_trace(None, None, None, 0, None, None, None, ctypes.byref(ar), None) == INVALID_ARG
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert bytes(wr) == bytes(ctypes.sizeof(wr)) and bytes(ar) == bytes(ctypes.sizeof(ar))   # nothing of the caller's was written
