"""The operand array of the paired product (tests/product_pairs.py, what tests/test_gpu_product_pairs.py feeds to the device), checked on
the CPU: every class and corner of the product chain in slot A against every one in slot B, so that all four combinations of
(A repairs, B repairs) occur, under every lane pattern; the portable `gl::mul_lazy2` (host build) gives the very lazy words of two
`gl::mul_lazy` on it, and `sbox_lazy2` the values of two `sbox_lazy`; the Poseidon states put (repair, none), (none, repair) and
(both) on the partners of every first-round pair. CPU only."""
import collections
import ctypes

import numpy as np
import pytest

import product_chain as C
import product_pairs as PP
import rare_paths as R

P = C.P
p64 = ctypes.POINTER(ctypes.c_uint64)


def ptr(x):
    return x.ctypes.data_as(p64)


@pytest.fixture(scope="module")
def hs():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("pairs_hostsim"))
    lib.pairs_mul_lazy2.argtypes = [p64] * 8 + [ctypes.c_size_t]
    lib.pairs_sbox.argtypes = [p64] * 4 + [ctypes.c_size_t]
    return lib


def test_pair_array_holds_every_class_against_every_class_in_every_pattern():
    A, B, C_, D, blocks = PP.pair_array()
    assert len(blocks) == len(PP.KEYS) ** 2 * len(R.PATTERNS) and A.size == len(blocks) * PP.N == B.size == C_.size == D.size
    w, _ = C.witnesses()
    for key in PP.KEYS:                       # the witnesses are what their key says (16 per key: `chain` runs here, not per lane)
        for a, b in w[key]:
            assert key in PP.key_of(C.chain(a, b))
    wset = {key: set(w[key]) for key in PP.KEYS}
    seen = collections.Counter()
    combos = collections.defaultdict(set)
    for ka, kb, name, off, mask in blocks:
        idx = off + np.nonzero(mask)[0]
        assert idx.size >= 16, (ka, kb, name)  # lane0 of 1024 lanes: one per wave
        assert all((int(a), int(b)) in wset[ka] for a, b in zip(A[idx], B[idx])), (ka, kb, name)
        assert all((int(c), int(d)) in wset[kb] for c, d in zip(C_[idx], D[idx])), (ka, kb, name)
        seen[(ka, kb, name)] += 1
        combos[name].add((PP.repairs(ka), PP.repairs(kb)))
    assert all(seen[(ka, kb, name)] == 1 for ka in PP.KEYS for kb in PP.KEYS for name in R.PATTERNS)
    for name in R.PATTERNS:
        assert combos[name] == {(False, False), (False, True), (True, False), (True, True)}, name


def test_portable_mul_lazy2_is_two_mul_lazy_on_the_pair_array(hs):
    A, B, C_, D, _ = PP.pair_array()
    n = A.size
    r0, r1, m0, m1 = (np.zeros(n, np.uint64) for _ in range(4))
    hs.pairs_mul_lazy2(ptr(A), ptr(B), ptr(C_), ptr(D), ptr(r0), ptr(r1), ptr(m0), ptr(m1), n)
    assert (r0 == m0).all() and (r1 == m1).all()   # the same lazy words, not only the same classes
    want_ab, want_cd = PP.pair_products()
    canon = lambda x: np.where(x >= np.uint64(P), x - np.uint64(P), x)
    assert (canon(r0) == want_ab).all() and (canon(r1) == want_cd).all()


def test_portable_sbox_lazy2_is_two_sbox_lazy(hs):
    A, _, C_, _, _ = PP.pair_array()
    x, y = A[::64].copy(), C_[::64].copy()          # lazy inputs (any u64), witnesses of every class among them
    x0, y0 = x.copy(), y.copy()
    sx, sy = np.zeros_like(x), np.zeros_like(y)
    hs.pairs_sbox(ptr(x), ptr(y), ptr(sx), ptr(sy), x.size)
    assert (x == sx).all() and (y == sy).all()
    assert x.tolist() == [pow(v, 7, P) for v in x0.tolist()] and y.tolist() == [pow(v, 7, P) for v in y0.tolist()]


def test_poseidon_pair_states_put_every_combination_on_every_pair_position():
    st, what = PP.poseidon_pair_states()
    assert st.shape == (256, 12) and (st < np.uint64(P)).all()
    assert {(q, combo) for _, q, combo in what} == {(q, combo) for q in range(PP.PAIR_POSITIONS) for combo in PP.COMBOS}
    for r, q, combo in what:
        for i in range(R.W):
            ch = PP.first_squaring(st, r, i)
            want = combo[i - 2 * q] if i // 2 == q else 0
            assert ch.borrow == want and (not want or ch.cy == 1), (r, i, q, combo)
