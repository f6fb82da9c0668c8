"""What tests/test_recombine_small_top.py (host) and tests/test_gpu_recombine_small_top.py (device) share: the libraries of
tests/recombine_sim, the tables of `recombine_s` decoded from the generated header, limb pairs whose fold wraps (or just does not),
and the seeded states of the k_permute test."""
import ctypes
import functools
import os
import re
import sys

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "city-rollup_amd", "csrc")
sys.path.insert(0, CSRC)
P = O.P
EPS = (1 << 32) - 1
p64 = ctypes.POINTER(ctypes.c_uint64)
pd = ctypes.POINTER(ctypes.c_double)
B1 = (0x433 << 52) + (1 << 51)          # bit pattern of 1.5 * 2^52
B32 = (0x413 << 52) + (1 << 51)         # of 1.5 * 2^20
# table id of rs_recombine -> (name in the header, name of its literal, bit pattern of the magic constant, limbs arrive in units of 2^32)
TABLES = {0: ("POSEIDON_RCS", "FULL", B1, False), 1: ("POSEIDON_DOMS_K", "PARTIAL", B1, False), 2: ("POSEIDON_DOMS_LAST", "PARTIAL", B1, False),
          3: ("POSEIDON_DOMS32_K", "PARTIAL32", B32, True), 4: ("POSEIDON_DOMS32_LAST", "PARTIAL32", B32, True)}
PERMUTE_SEED, PERMUTE_COUNT = 0x5EED0A11, 1 << 16


def host_lib(kind="host"):
    import simlibs
    lib = ctypes.CDLL(simlibs.build("recombine_" + kind))
    lib.rs_top0.restype = ctypes.c_uint32
    lib.rs_recombine.restype = ctypes.c_uint64
    lib.rs_recombine.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int)]
    lib.rs_top.restype = ctypes.c_uint32
    lib.rs_top.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    lib.rs_site.argtypes = [ctypes.c_int, ctypes.c_int, pd, pd, p64, ctypes.c_size_t]
    lib.rs_permute.argtypes = [p64, ctypes.c_size_t, ctypes.c_int]
    lib.rs_wrap_runs.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lib.rs_matrix.argtypes = [ctypes.c_int, pd]
    lib.rs_dom.argtypes = [ctypes.c_int, pd, pd]
    lib.rs_trip.argtypes = [ctypes.c_int, pd, pd, pd, pd, pd]
    return lib


@functools.lru_cache(maxsize=None)
def parse_table(name):
    src = open(os.path.join(CSRC, "poseidon_tables.h")).read()
    m = re.search(r"%s\[\d+\] = \{(.*?)\};" % name, src, re.S)
    return [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)", m.group(1))]


@functools.lru_cache(maxsize=None)
def parse_literal(name):
    src = open(os.path.join(CSRC, "poseidon_tables.h")).read()
    return int(re.search(r"POSEIDON_TOP0_%s = 0x([0-9a-fA-F]+)u;" % name, src).group(1), 16)


def halves(table, i):
    """(lo32, hi32) of the stored constant of entry i: the mantissas of its two doubles"""
    name, _, B, _ = TABLES[table]
    bits = parse_table(name)[2 * i:2 * i + 2]
    assert all(B <= b < B + (1 << 32) for b in bits)
    return bits[0] - B, bits[1] - B


def wanted_constants():
    """table id -> the constants the entries must add, from gen_tables"""
    import gen_tables as G
    rc = G.round_constants()
    dk, dlast = G.plane_constants(rc, first_too=True)
    return {0: rc + [0], 1: dk, 2: dlast, 3: dk, 4: dlast}


def as_arg(table, v):
    """a limb (integer, units of 1) as the double the table's form takes"""
    return float(v) / 4294967296.0 if TABLES[table][3] else float(v)


def top_of(table, i, l, h):
    """the top word and the 64 low bits of `recombine_s` on integer limbs, with Python integers"""
    _, lit, B, _ = TABLES[table]
    c0, c1 = halves(table, i)
    a0, a1 = B + l + c0, B + h + c1
    mid = (a0 >> 32) + (a1 & EPS)
    return (a1 >> 32) + (mid >> 32) - parse_literal(lit), ((mid & EPS) << 32) | (a0 & EPS)


def wrap_pair(table, i, l, k, wraps=True):
    """for a low limb l, the high limb h = ... + k 2^32 whose middle word is all ones (the fold then wraps as soon as top >= 2), or,
    wraps=False, a middle word just too small for it: 2^32 - 2 - top"""
    _, _, B, _ = TABLES[table]
    c0, c1 = halves(table, i)
    hi_a0 = ((B + l + c0) >> 32) & EPS
    h = ((EPS - hi_a0 - c1) % (1 << 32)) + (k << 32)
    if not wraps:
        top, _ = top_of(table, i, l, h)
        h -= top + 1                      # middle word 2^32 - 2 - top: lo + top (2^32 - 1) < 2^64 whatever the low word
        assert top_of(table, i, l, h)[0] in (top, top - 1)
    top, lo = top_of(table, i, l, h)
    assert (lo + top * EPS >= 1 << 64) == wraps, (table, i, l, k)
    return h


def permute_states():
    return O.splitmix64_felts(PERMUTE_SEED, 12 * PERMUTE_COUNT).reshape(-1, 12).copy()
