"""The recombination with a small top word on the device (poseidon.h `recombine_s` / `repair_s`: carry-outs in SGPR pairs, one
wave-uniform test per group, the repair behind it) under every lane pattern of (wraps, does not wrap), and the kernels that run it
with the triangular b block (k_permute, hash_no_pad, the leaf hash and the level kernels), byte for byte against the host form and the
CPU oracle. The GPU is touched only inside tests."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O
import recombine_cases as RC
from recombine_cases import P, p64, pd

pytestmark = pytest.mark.gpu
LANE = {"COOP_LEAF_MAX": 0, "COOP_MAX": 0}     # the lane-per-leaf / lane-per-parent kernels at every size
N = 320                                        # five waves over two workgroups, the second one partial


@pytest.fixture(scope="module")
def libs():
    import simlibs
    dev = ctypes.CDLL(simlibs.build("recombine_device"))
    dev.rsd_site.argtypes = [ctypes.c_int, ctypes.c_int, pd, pd, p64, ctypes.c_size_t]
    return RC.host_lib("host"), dev, RC.wanted_constants()


# which (element, position) wrap. Elements are lanes: 64 to a wave.
PATTERNS = {
    "no_lane": lambda e, k: False,
    "one_lane": lambda e, k: e == 37,
    "one_lane_one_position": lambda e, k: e == 200 and k == 7,
    "all_lanes": lambda e, k: True,
    "alternating_lanes": lambda e, k: e % 2 == 1,
    "alternating_positions": lambda e, k: (e + k) % 2 == 0,
    "last_lane_of_each_wave": lambda e, k: e % 64 == 63,
}
for _k in range(12):
    PATTERNS["position_%d" % _k] = (lambda kk: lambda e, k: k == kk and e % 3 == 0)(_k)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_device_recombine_under_lane_patterns(libs, pattern):
    hs, dev, consts = libs
    wraps = PATTERNS[pattern]
    for site, table, idx in ((0, 0, 3), (2, 4, 0), (1, 3, 9)):
        cnt = 1 if site == 1 else 12
        l = np.zeros((N, 12))
        h = np.zeros((N, 12))
        want_mod = np.zeros((N, 12), object)
        for e in range(N):
            for k in range(cnt):
                i = idx * 12 + k if table == 0 else (idx if site == 1 else k)
                li = 7919 * e + 13 * k if table == 0 else (-1) ** e * (7919 * e + 13 * k)
                hi = RC.wrap_pair(table, i, li, 5 if table == 0 else (e % 7) - 3, wraps=bool(wraps(e, k)))
                l[e, k], h[e, k] = RC.as_arg(table, li), RC.as_arg(table, hi)
                want_mod[e, k] = (li + (hi << 32) + consts[table][i]) % P
        sentinel = np.uint64(0x5E5E5E5E5E5E5E5E)
        host = np.full((N, 12), sentinel, np.uint64)
        got = host.copy()
        hs.rs_site(site, idx, l.ctypes.data_as(pd), h.ctypes.data_as(pd), host.ctypes.data_as(p64), N)
        if site == 1:
            host[:, 1:] = sentinel            # the host form writes the whole row; the device leaves what it does not own
        assert dev.rsd_site(site, idx, l.ctypes.data_as(pd), h.ctypes.data_as(pd), got.ctypes.data_as(p64), N) == 0
        assert (got == host).all(), (pattern, site)
        assert all(int(got[e, k]) % P == want_mod[e, k] for e in range(N) for k in range(cnt)), (pattern, site)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def test_permute_kernel_on_the_seeded_states(prover):
    """2^16 states; tests/test_recombine_small_top.py::test_seeded_states_take_the_rare_path shows on the host form that they take the
    repair in a partial round and at the exit of the partial rounds, and that no full-round layer wraps for them (its top word is at
    most 266: a 2^-24 event per word) — that site is driven by the lane patterns above."""
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    try:
        st = RC.permute_states()
        assert (prover.poseidon_permute(st) == O.permute_many(st).reshape(-1, 12)).all()
    finally:
        O.lib().or_set_threads(1)


@pytest.mark.parametrize("length", [9, 135])
def test_hash_no_pad(prover, length):
    x = O.splitmix64_felts(0xA5 + length, 64 * length).reshape(64, length)
    got = prover.hash_no_pad(x)
    assert all((got[i] == O.hash_no_pad(x[i])).all() for i in range(64))


_trees = {}


def tree_case(leaf_len, cap_h):
    if (leaf_len, cap_h) not in _trees:
        cols = O.splitmix64_felts(0x51AB + 10 * leaf_len + cap_h, leaf_len << 9).reshape(leaf_len, -1)
        _trees[(leaf_len, cap_h)] = (cols,) + tuple(O.merkle_tree_cols(cols, cap_h, want_digests=True))
    return _trees[(leaf_len, cap_h)]


@pytest.mark.parametrize("fuse", [0, 1])
def test_tree_of_512_leaves_in_every_digest(fuse):
    import cityprover
    p = cityprover.Prover(0)
    try:
        for k, v in dict(LANE, MERKLE_FUSE=fuse).items():
            p.set_option(k, v)
        for leaf_len in (9, 135):
            for cap_h in (0, 4):
                cols, want_cap, want_dig = tree_case(leaf_len, cap_h)
                cap, dig = p.merkle_cols(cols, cap_h, want_digests=True)
                assert (cap == want_cap).all(), (fuse, leaf_len, cap_h)
                assert (dig == want_dig).all(), ("digests", fuse, leaf_len, cap_h)
    finally:
        p.close()
