"""ctypes loader for the bench-side witness helper (tools/witgen/witgen.hip)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libwitgen.so")
_lib = None


def build():
    """Compile libwitgen.so if missing or stale (cityprover.build.compile_if_needed; several ranks may get here at once)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "city-rollup_amd"))
    from cityprover.build import compile_if_needed
    return compile_if_needed(os.path.join(HERE, "witgen.hip"), SO, ["--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-Wno-unused-value"], "-shared")


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def poseidon_gate_rows(inputs, swaps):
    inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
    swaps = np.ascontiguousarray(swaps, dtype=np.uint64)
    n = inputs.shape[0]
    out = np.zeros((n, 135), np.uint64)
    p = ctypes.POINTER(ctypes.c_uint64)
    lib().wg_poseidon_gate_rows(inputs.ctypes.data_as(p), swaps.ctypes.data_as(p), ctypes.c_size_t(n),
                                out.ctypes.data_as(p))
    return out
