"""The lane-per-leaf hash and the node kernels with the sponge-aware permutation forms (poseidon.h `permute_until<OUT, ZERO_CAP>`;
merkle.h k_leaf_hash_cols: capacity only while the next chunk is whole, everything before a partial last chunk, digest at the
end; nodes: zero capacity in, digest out) against the CPU oracle, in every digest and the cap. (A salted tree lives in a
PolyBatch, which hands out its cap and its leaves but no digests: there the cap at height 0, the root over every digest, stands
for them.)

The lane-per-leaf kernels are forced through the existing switches (COOP_LEAF_MAX = 0, COOP_MAX = 0, MERKLE_FUSE 0..3) on a private
context. Leaf lengths: 4 = not hashed; 5 = one permutation that is first and last; 8 = exactly one whole chunk; 9 = whole +
partial; 16 = two whole; 17 = two whole + partial; 135 = the workload's own (15 capacity-only, one full, one digest). Salt (4
words) moves the chunk boundaries: 5 + 4 and 8 + 4. 256 and 1024 leaves are one and four workgroups; 2^14 leaves run under the
default switches. The GPU is touched only inside tests."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
SALT = 4
LANE = {"COOP_LEAF_MAX": 0, "COOP_MAX": 0}
LEAF_LENS = (4, 5, 8, 9, 16, 17, 135)
VALUES = ("random", "zero", "p-1")


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    yield
    O.lib().or_set_threads(1)


def forced(opts):
    import cityprover
    p = cityprover.Prover(0)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def fill(kind, seed, shape):
    if kind == "zero":
        return np.zeros(shape, np.uint64)
    if kind == "p-1":
        return np.full(shape, P - 1, np.uint64)
    return O.splitmix64_felts(seed, int(np.prod(shape))).reshape(shape).copy()


_oracle = {}


def tree_case(n_leaves, leaf_len, cap_h, kind):
    """computed once, shared by the four MERKLE_FUSE rows, never modified"""
    key = (n_leaves, leaf_len, cap_h, kind)
    if key not in _oracle:
        cols = fill(kind, 0x1EAF0000 + 4096 * leaf_len + 8 * cap_h + n_leaves, (leaf_len, n_leaves))
        cols.setflags(write=False)
        _oracle[key] = (cols,) + tuple(O.merkle_tree_cols(cols, cap_h, want_digests=True))
    return _oracle[key]


@pytest.mark.parametrize("cap_h", [0, 4])
@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
def test_lane_per_leaf_tree_matches_oracle_in_every_digest(fuse, cap_h):
    p = forced(dict(LANE, MERKLE_FUSE=fuse))
    try:
        for n_leaves in (256, 1024):
            for leaf_len in LEAF_LENS:
                for kind in VALUES:
                    cols, want_cap, want_dig = tree_case(n_leaves, leaf_len, cap_h, kind)
                    p.profile_begin()
                    try:
                        cap, dig = p.merkle_cols(cols, cap_h, want_digests=True)
                    finally:
                        prof = p.profile_end()
                    assert prof["leaf_hash_cols"]["launches"] == 1 and "leaf_hash_cols_coop" not in prof, (n_leaves, leaf_len)
                    assert "merkle_level_coop" not in prof and "merkle_levels_coop" not in prof, (n_leaves, leaf_len)
                    assert (dig == want_dig).all(), ("digests", fuse, cap_h, n_leaves, leaf_len, kind)
                    assert (cap == want_cap).all(), ("cap", fuse, cap_h, n_leaves, leaf_len, kind)
    finally:
        p.close()


@pytest.mark.parametrize("cap_h", [0, 4])
def test_default_planner_at_2_to_14_leaves(cap_h):
    """switches at their defaults: 2^14 leaves are past the twelve-lane form, the planner's own choice of fused levels runs"""
    p = forced({})
    try:
        for leaf_len in (9, 135):
            cols, want_cap, want_dig = tree_case(1 << 14, leaf_len, cap_h, "random")
            p.profile_begin()
            try:
                cap, dig = p.merkle_cols(cols, cap_h, want_digests=True)
            finally:
                prof = p.profile_end()
            assert prof["leaf_hash_cols"]["launches"] == 1, sorted(prof)
            assert (dig == want_dig).all(), ("digests", cap_h, leaf_len)
            assert (cap == want_cap).all(), ("cap", cap_h, leaf_len)
    finally:
        p.close()


@pytest.mark.parametrize("cap_h", [0, 4])
@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
def test_three_trees_per_call(fuse, cap_h):
    """commit_batch_dev with three trees: blockIdx.y strides of the leaf hash, the fused levels and the level kernel"""
    trees, rate = 3, 3
    p = forced(dict(LANE, MERKLE_FUSE=fuse))
    try:
        for log_n in (5, 7):          # 256 and 1024 leaves
            for k in LEAF_LENS:
                for kind in VALUES:
                    n = 1 << log_n
                    N = n << rate
                    vals = fill(kind, 0x7EE5 + 64 * k + log_n, (trees * k, n))
                    per_tree = 2 * N - (2 << cap_h)
                    dv, dl, dd, dcap = p.to_device(vals), p.alloc(trees * k * N), p.alloc(trees * per_tree * 4), p.alloc(trees * (4 << cap_h))
                    try:
                        p.commit_batch_dev(dv.ptr, k, trees, log_n, rate, cap_h, dl.ptr, dcap.ptr, None, dd.ptr)
                        dig = dd.download().reshape(trees, per_tree, 4)
                        caps = dcap.download().reshape(trees, 1 << cap_h, 4)
                    finally:
                        for b in (dv, dl, dd, dcap):
                            b.free()
                    for t in range(trees):
                        key = ("batch", log_n, k, cap_h, kind, t)
                        if key not in _oracle:
                            _oracle[key] = O.commit_batch(vals[t * k:(t + 1) * k], rate, cap_h, want=("cap", "digests"))
                        want = _oracle[key]
                        assert (dig[t] == want["digests"]).all(), ("digests", fuse, cap_h, log_n, k, kind, t)
                        assert (caps[t] == want["cap"]).all(), ("cap", fuse, cap_h, log_n, k, kind, t)
    finally:
        p.close()


@pytest.mark.parametrize("cap_h", [0, 4])
@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
def test_salted_leaves(fuse, cap_h):
    """k_leaf_hash_cols<true, F>: 5 + 4 words (whole + partial chunk) and 8 + 4 (the salt starts the second chunk). A batch
    exposes no digests; the cap of height 0 is the root over all of them, the cap of height 4 over all below it."""
    import cityprover
    rate = 3
    p = forced(dict(LANE, MERKLE_FUSE=fuse))
    try:
        for log_n in (5, 7):
            for k in (5, 8):
                for kind in VALUES:
                    n = 1 << log_n
                    N = n << rate
                    polys = fill(kind, 0x5A17 + 16 * k + log_n, (k, n))
                    salts = fill(kind, 0x5A18 + 16 * k + log_n, (SALT, N))
                    ob = O.Batch(polys, rate, cap_h, salts=salts)
                    gb = cityprover.PolyBatch(p, polys, rate, cap_h, salts=salts)
                    try:
                        assert (gb.cap() == ob.cap()).all(), (fuse, cap_h, log_n, k, kind)
                        assert (gb.leaves(0, N) == ob.lde().T).all(), (fuse, cap_h, log_n, k, kind)
                    finally:
                        gb.close()
                        ob.close()
    finally:
        p.close()
