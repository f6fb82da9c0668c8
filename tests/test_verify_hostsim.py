"""csrc/fri_verify.h compiled for the host (tests/verify_hostsim): check_path and check_query, the code the kernels of
cp_verify_batch run per lane, against the oracle's Merkle verifier, the ten reference proofs with their recovered challenges, and
the refusals of the host verifier on mutated copies. CPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import reference_challenges as R
import verify_batch_cases as V

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "city-rollup_amd"))
P = O.P
_u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def vh():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("verify_hostsim"))
    lib.vh_instance_size.restype = ctypes.c_size_t
    lib.vh_check_path.argtypes = [_u64p, ctypes.c_uint32, ctypes.c_uint64, _u64p, ctypes.c_uint32, _u64p, ctypes.c_uint32]
    lib.vh_query_phase.restype = ctypes.c_uint32
    lib.vh_query_phase.argtypes = [ctypes.POINTER(V.Instance), _u64p, _u64p, _u64p]
    lib.vh_coset_eval.argtypes = [_u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, _u64p, _u64p]
    assert lib.vh_instance_size() == ctypes.sizeof(V.Instance)
    return lib


def ptr(a):
    return a.ctypes.data_as(_u64p)


def tree_paths(leaves, cap_height):
    """(cap, [siblings of leaf i]) of the oracle's tree over `leaves`"""
    n = len(leaves)
    level = [O.hash_or_noop(leaves[i]) for i in range(n)]
    levels = []
    while len(level) > (1 << cap_height):
        levels.append(level)
        level = [O.two_to_one(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
    cap = np.array(level, dtype=np.uint64).reshape(-1, 4)
    sib = [[[int(v) for v in lv[(i >> d) ^ 1]] for d, lv in enumerate(levels)] for i in range(n)]
    return cap, sib


@pytest.mark.parametrize("cap_height", [3, 1])     # depth 0 (eight leaves, eight cap entries) and depth 2
def test_check_path_edges(vh, cap_height):
    """leaves of 1 .. 20 elements: both sides of the noop boundary at 4 and of the chunk boundaries at 8 and 16"""
    n = 8
    depth = 3 - cap_height
    for leaf_len in range(1, 21):
        leaves = O.splitmix64_felts(100 * cap_height + leaf_len, n * leaf_len).reshape(n, leaf_len)
        cap, sibs = tree_paths(leaves, cap_height)
        assert (cap == np.asarray(O.merkle_tree(leaves, cap_height), dtype=np.uint64).reshape(-1, 4)).all()
        for i in (0, 5, 7):
            sib = np.array(sibs[i], dtype=np.uint64).reshape(-1)
            sib = np.concatenate([sib, np.zeros(4, np.uint64)])      # never empty
            leaf = np.ascontiguousarray(leaves[i])
            args = lambda lf, ix, sb, cp: (ptr(lf), leaf_len, ix, ptr(sb), depth, ptr(cp), cap_height)
            assert O.merkle_verify(leaf, i, sibs[i], cap, cap_height)
            assert vh.vh_check_path(*args(leaf, i, sib, cap)) == 1, (leaf_len, i)
            bad = leaf.copy()
            bad[leaf_len - 1] = (int(bad[leaf_len - 1]) + 1) % P
            assert not O.merkle_verify(bad, i, sibs[i], cap, cap_height)
            assert vh.vh_check_path(*args(bad, i, sib, cap)) == 0, (leaf_len, i)
            assert vh.vh_check_path(*args(leaf, i + n, sib, cap)) == 0              # an index past the cap
            assert vh.vh_check_path(*args(leaf, i ^ (1 << depth), sib, cap)) == 0   # another cap entry
            if depth:
                wrong = sib.copy()
                wrong[4 * (depth - 1) + 2] ^= 1
                ws = [list(s) for s in sibs[i]]
                ws[depth - 1][2] ^= 1
                assert not O.merkle_verify(leaf, i, ws, cap, cap_height)
                assert vh.vh_check_path(*args(leaf, i, wrong, cap)) == 0           # a wrong sibling
                assert vh.vh_check_path(*args(leaf, i ^ 1, sib, cap)) == 0          # the sibling's side


@pytest.mark.parametrize("ab", [1, 2, 3, 4, 5])
def test_coset_eval_is_the_interpolant(vh, ab):
    """compute_evaluation without a per-lane array against Lagrange interpolation on Python integers, every position in the coset"""
    n = 1 << ab
    rng = np.random.default_rng(ab)
    x = int(rng.integers(1, 2**62))
    beta = (int(rng.integers(0, 2**62)), int(rng.integers(0, 2**62)))
    evals = O.splitmix64_felts(7 + ab, 2 * n)
    pairs = [(int(evals[2 * i]), int(evals[2 * i + 1])) for i in range(n)]
    b = np.array(beta, dtype=np.uint64)
    for within in sorted({0, 1, n - 1, n // 2}):
        out = np.zeros(2, np.uint64)
        vh.vh_coset_eval(ptr(evals), x, within, ab, V.root(ab), ptr(b), ptr(out))
        want = R.peval(R.fold_poly(x, within, ab, pairs), beta)
        assert (int(out[0]), int(out[1])) == want, within


def run(vh, cp, sh, blob, args):
    D, words = V.layout(sh)
    assert len(blob) == 8 * words
    from proof_format import parse_proof
    rec = V.record(sh, parse_proof(blob), *args)
    pw = np.frombuffer(blob, dtype=np.uint64).copy()
    return V.key_triple(D, vh.vh_query_phase(ctypes.byref(D), ptr(pw), ptr(rec), None))


@pytest.mark.parametrize("which", range(10))
def test_reference_proofs_accepted(vh, golden_dir, which):
    """every path and every check_query of a reference proof, folded into the key as the kernels do"""
    import cityprover as cp
    blob, pf, ch = R.challenges(golden_dir, which)
    sh = cp.standard_recursion_shape(num_public_inputs=len(pf["public_inputs"]))
    assert run(vh, cp, sh, blob, (ch["alpha"], ch["zeta"], ch["betas"], ch["x_indices"])) == (0, -1, -1)


@pytest.mark.parametrize("which", [0, 1])
def test_mutations_name_the_host_verifiers_check(vh, golden_dir, which):
    """the eleven mutations of tests/test_reference_product_parity.py and a flipped index of the last query: wherever the host
    hook refuses, the key decodes to the check and the query its message names"""
    import cityprover as cp
    blob, pf, ch = R.challenges(golden_dir, which)
    sh = cp.standard_recursion_shape(num_public_inputs=len(pf["public_inputs"]))
    cases = V.reference_mutations(blob, (ch["alpha"], ch["zeta"], ch["betas"], ch["x_indices"]))
    assert len(cases) == 12
    refused = 0
    for name, bad, args in cases:
        try:
            cp.verify_fri_queries_with_challenges(sh, bad, *args)
        except cp.CityProverError as e:
            refused += 1
            assert run(vh, cp, sh, bad, args) == V.message_triple(str(e)), name
        else:
            assert run(vh, cp, sh, bad, args) == (0, -1, -1), name
    assert refused == 12
