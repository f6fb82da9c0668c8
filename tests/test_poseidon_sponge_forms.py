"""The sponge-aware forms of the permutation (poseidon.h `permute_until<OUT, ZERO_CAP>`: which outputs are kept, whether the
capacity comes in as zero) on the host: every live word equals `permute_textbook`'s. CPU only."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O

P = O.P
OUT_ALL, OUT_CAPACITY, OUT_DIGEST = 0, 1, 2
LIVE = {OUT_ALL: slice(0, 12), OUT_CAPACITY: slice(8, 12), OUT_DIGEST: slice(0, 4)}
p64 = ctypes.POINTER(ctypes.c_uint64)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def hs():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("sponge_hostsim"))
    lib.hs_sponge_permute.argtypes = [p64, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    lib.hs_sponge_node.argtypes = [p64, ctypes.c_uint64, p64]
    lib.hs_sponge_textbook.argtypes = [p64, ctypes.c_size_t]
    lib.hs_sponge_hash.argtypes = [p64, ctypes.c_int, ctypes.c_uint64, p64]
    lib.hs_sponge_hash_textbook.argtypes = [p64, ctypes.c_int, p64]
    return lib


def input_states():
    """random canonical states; all zero; all p - 1; rows of boundary words; lazy words near 2^64 on the capacity (what a
    capacity-only permutation hands to the next one) and everywhere"""
    rng = np.random.default_rng(17)
    st = O.splitmix64_felts(0x5F0A6E, 12 * 96).reshape(-1, 12).copy()
    st[0] = 0
    st[1] = P - 1
    edge = np.array([0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 1 << 63], np.uint64)
    for i in range(2, 24):
        st[i] = rng.choice(edge, 12)
    lazy = np.array([M64, M64 - 1, M64 - 0xFFFFFFFF, (1 << 64) - (1 << 32), P, P + 1, M64 - 0xFFFFFFFE], np.uint64)
    for i in range(24, 48):
        st[i, 8:] = rng.choice(lazy, 4)
    for i in range(48, 56):
        st[i] = rng.choice(lazy, 12)
    st[56, 8:] = M64
    return st


def textbook(hs, st):
    want = st.copy()
    hs.hs_sponge_textbook(want.ctypes.data_as(p64), want.shape[0])
    return want


@pytest.mark.parametrize("zero_cap", [0, 1], ids=["any_capacity", "zero_capacity"])
@pytest.mark.parametrize("out", [OUT_ALL, OUT_CAPACITY, OUT_DIGEST], ids=["all", "capacity", "digest"])
def test_live_words_equal_textbook(hs, out, zero_cap):
    st = input_states()
    ref_in = st.copy()
    if zero_cap:
        ref_in[:, 8:] = 0
        st[::2, 8:] = 0                                   # either truly zero ...
        st[1::2, 8:] = np.uint64(0xDEADBEEFDEADBEEF)      # ... or never read: the flag is a promise about the value, not a load
    want = textbook(hs, ref_in)
    assert (want == O.permute_many(ref_in % np.uint64(P)).reshape(-1, 12)).all()   # the textbook form is the oracle's
    got = st.copy()
    assert hs.hs_sponge_permute(got.ctypes.data_as(p64), got.shape[0], out, zero_cap) == 0
    live = LIVE[out]
    if out == OUT_CAPACITY:   # left lazy: any u64 congruent to the value
        assert ((got[:, live] % np.uint64(P)) == want[:, live]).all()
    else:                     # canonical
        assert (got[:, live] == want[:, live]).all()


def test_chain_of_17_capacity_only_permutations(hs):
    """17 capacity-only permutations in a row, fresh rate words each time (the middle of a 135-column leaf), against 17
    textbook permutations: the lazy capacity words are carried from one to the next."""
    rng = np.random.default_rng(23)
    n = 32
    chunks = O.splitmix64_felts(99, 17 * n * 8).reshape(17, n, 8)
    chunks[3] = P - 1
    chunks[4] = 0
    a = np.zeros((n, 12), np.uint64)
    a[:, 8:] = rng.integers(0, P, (n, 4), dtype=np.uint64)
    b = a.copy()
    for c in range(17):
        a[:, :8] = chunks[c]
        b[:, :8] = chunks[c]
        assert hs.hs_sponge_permute(a.ctypes.data_as(p64), n, OUT_CAPACITY, 0) == 0
        a[:, :8] = np.uint64(0xA5A5A5A5A5A5A5A5)   # dead words: nothing may depend on them
        hs.hs_sponge_textbook(b.ctypes.data_as(p64), n)
        assert ((a[:, 8:] % np.uint64(P)) == b[:, 8:]).all(), c


@pytest.mark.parametrize("total", [5, 7, 8, 9, 12, 16, 17, 23, 24, 135, 136, 143])
def test_sponge_as_the_leaf_kernels_run_it(hs, total):
    """hash_no_pad with one call per form (capacity only while the next chunk is whole, everything before a partial last chunk,
    digest at the end) equals the plain sponge over the textbook permutation and the oracle's hash."""
    for seed, fill in ((1, None), (2, 0), (3, P - 1)):
        w = O.splitmix64_felts(seed * 1000 + total, total).copy()
        if fill is not None:
            w[:] = fill
        got, want = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        hs.hs_sponge_hash(w.ctypes.data_as(p64), total, 0xDEADBEEFDEADBEEF, got.ctypes.data_as(p64))
        hs.hs_sponge_hash_textbook(w.ctypes.data_as(p64), total, want.ctypes.data_as(p64))
        assert (got == want).all()
        assert (got == O.hash_no_pad(w)).all()


def test_node_permutation_is_two_to_one(hs):
    d = O.splitmix64_felts(77, 8 * 40).reshape(-1, 8).copy()
    d[0] = 0
    d[1] = P - 1
    for row in d:
        got = np.zeros(4, np.uint64)
        hs.hs_sponge_node(row.ctypes.data_as(p64), 0xDEADBEEFDEADBEEF, got.ctypes.data_as(p64))
        assert (got == O.two_to_one(row[:4], row[4:])).all()
