"""cp_verify_batch and cp_verify_fri_queries_with_challenges_batch at the boundary, without a GPU: what is wrong with a call is a
status and a message, never a crash, and the second one refuses exactly the shapes the host hook refuses."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "city-rollup_amd"))
INVALID = -1   # CP_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def cp():
    import cityprover
    cityprover.load_library()
    return cityprover


def last(cp):
    return cp.load_library().cp_last_error(None).decode()


def batch_call(cp, shape, n=1, ctx=None, drop=()):
    """the second entry point with one well-formed set of arguments; `drop` names the pointers passed as NULL"""
    lib = cp.load_library()
    nq, nl = max(shape.num_query_rounds, 1), max(shape.n_arity, 0)
    blob = b"\0" * 64
    keep, ptrs, lens = cp._proof_array([blob] * max(n, 1))
    a, z, fb, xi = (np.zeros(k, np.uint64) for k in (2 * max(n, 1), 2 * max(n, 1), 2 * nl * max(n, 1) + 2, nq * max(n, 1)))
    out = np.zeros(max(n, 1), cp.VERDICT)
    args = dict(shape=ctypes.byref(shape), proofs=ptrs, lens=lens, alphas=cp._ptr(a), zetas=cp._ptr(z), betas=cp._ptr(fb), xi=cp._ptr(xi),
                out=out.ctypes.data)
    for name in drop:
        args[name] = None
    return lib.cp_verify_fri_queries_with_challenges_batch(ctx, args["shape"], None, args["proofs"], args["lens"], n, args["alphas"], args["zetas"],
                                                           args["betas"], args["xi"], 0, args["out"])


def test_abi_version_is_unchanged(cp):
    assert cp.load_library().cp_abi_version() == 4


def test_verify_batch_null_circuit(cp):
    lib = cp.load_library()
    keep, ptrs, lens = cp._proof_array([b"\0" * 8])
    out = np.zeros(1, cp.VERDICT)
    assert lib.cp_verify_batch(None, ptrs, lens, 1, 0, out.ctypes.data) == INVALID
    assert "circuit is NULL" in last(cp)
    assert lib.cp_verify_batch(None, None, None, 0, 0, None) == INVALID


def test_challenges_batch_null_arguments(cp):
    sh = cp.standard_recursion_shape()
    assert batch_call(cp, sh) == INVALID and "ctx is NULL" in last(cp)           # everything else is in order
    for name in ("shape", "proofs", "lens", "alphas", "zetas", "betas", "xi", "out"):
        assert batch_call(cp, sh, drop=(name,)) == INVALID, name
        assert "NULL argument" in last(cp), name
    assert batch_call(cp, sh, n=0) == INVALID and "no proofs" in last(cp)
    no_layers = cp.standard_recursion_shape(arity_bits=())
    assert batch_call(cp, no_layers, drop=("betas",)) == INVALID and "ctx is NULL" in last(cp)   # no beta to point at


BAD_SHAPES = [dict(degree_bits=1), dict(degree_bits=28), dict(rate_bits=-1), dict(num_challenges=0), dict(num_challenges=9),
              dict(arity_bits=(1,) * 9), dict(cap_height=-1), dict(cap_height=16), dict(num_query_rounds=0), dict(num_query_rounds=256),
              dict(num_wires=0), dict(num_constants=-1), dict(num_routed_wires=-1), dict(num_partial_products=-1),
              dict(quotient_degree_factor=0), dict(arity_bits=(0,)), dict(arity_bits=(4, 6))]


@pytest.mark.parametrize("over", BAD_SHAPES, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_challenges_batch_refuses_the_shapes_the_hook_refuses(cp, over):
    lib = cp.load_library()
    if len(over.get("arity_bits", ())) > 8:
        sh = cp.standard_recursion_shape()
        sh.n_arity = 9
    else:
        sh = cp.standard_recursion_shape(**over)
    z = np.zeros(64, np.uint64)
    assert lib.cp_verify_fri_queries_with_challenges(ctypes.byref(sh), b"\0" * 64, 64, cp._ptr(z), cp._ptr(z), cp._ptr(z), cp._ptr(z)) == INVALID
    hook = last(cp)
    assert "out of range" in hook
    assert batch_call(cp, sh) == INVALID
    assert last(cp) == hook
