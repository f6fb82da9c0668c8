"""The kernels that run the partial rounds in units of 2^32 (poseidon.h renorm32_d: k_permute, the leaf hash, the level kernel), byte for
byte against the CPU oracle. The GPU is touched only inside tests."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
SALT = 4
EDGE = np.array([0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 1 << 63, P >> 1, 7], dtype=np.uint64)
# the lane-per-leaf leaf hash and the lane-per-parent level kernel at every size (the twelve-lane kernels do not run partial_rounds)
LANE = {"COOP_LEAF_MAX": 0, "COOP_MAX": 0}


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    yield
    O.lib().or_set_threads(1)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def forced(opts):
    import cityprover
    p = cityprover.Prover(0)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def test_permute_kernel_on_random_and_edge_states(prover):
    rng = np.random.default_rng(41)
    st = O.splitmix64_felts(0x9E27, 12 * 4096).reshape(-1, 12).copy()
    st[0] = 0
    st[1] = P - 1
    for i in range(2, 600):
        st[i] = rng.choice(EDGE, 12)
    assert (prover.poseidon_permute(st) == O.permute_many(st).reshape(-1, 12)).all()


_trees = {}


def tree_case(log_n, leaf_len, cap_h):
    key = (log_n, leaf_len, cap_h)
    if key not in _trees:
        cols = O.splitmix64_felts(0x7AB1E + 1000 * log_n + 10 * leaf_len + cap_h, leaf_len << log_n).reshape(leaf_len, -1)
        _trees[key] = (cols,) + tuple(O.merkle_tree_cols(cols, cap_h, want_digests=True))
    return _trees[key]


@pytest.mark.parametrize("fuse", [0, 1])
def test_merkle_trees_in_every_digest(fuse):
    """leaf lengths 7 (one partial chunk), 8, 16 (whole chunks), 9, 135 (whole chunks and a partial last one: both sponge forms)"""
    import cityprover
    p = forced(dict(LANE, MERKLE_FUSE=fuse))
    try:
        for log_n in (10, 12):
            for leaf_len in (7, 8, 9, 16, 135):
                for cap_h in (0, 4):
                    cols, want_cap, want_dig = tree_case(log_n, leaf_len, cap_h)
                    cap, dig = p.merkle_cols(cols, cap_h, want_digests=True)
                    assert (cap == want_cap).all(), (fuse, log_n, leaf_len, cap_h)
                    assert (dig == want_dig).all(), ("digests", fuse, log_n, leaf_len, cap_h)
        # salted once: 2^10 leaves of 5 + 4 words
        log_n, rate, k, cap_h = 7, 3, 5, 4
        rng = np.random.default_rng(77)
        polys = rng.integers(0, P, (k, 1 << log_n), dtype=np.uint64)
        salts = rng.integers(0, P, (SALT, 1 << (log_n + rate)), dtype=np.uint64)
        ob = O.Batch(polys, rate, cap_h, salts=salts)
        gb = cityprover.PolyBatch(p, polys, rate, cap_h, salts=salts)
        try:
            assert (gb.cap() == ob.cap()).all(), ("salted", fuse)
        finally:
            gb.close()
            ob.close()
    finally:
        p.close()
