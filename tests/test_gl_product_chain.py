"""The carry-aware product chain of csrc/gl.h with Python integers (tests/product_chain.py): congruent to a b mod p, and its four
bounds hold as assertions inside `chain` — hi' cannot carry, hi32(hi') + cy stays below 2^32 (also after mul_add_lazy's + 1), the
repaired t0 cannot underflow, the fold cannot wrap twice — over edge pairs, the 16^4 half-word operands, random pairs and the
operands rare_paths builds. Also: the witness array of tests/test_gpu_product_chain.py reaches all twelve classes of
(cy, low-word borrow, 64-bit borrow, fold wrap) and the two corners that only the carry-in creates. CPU only."""
import numpy as np

import product_chain as C
import rare_paths as R

P = C.P


def test_chain_on_every_pair_of_edge_values():
    for a in C.EDGE:
        for b in C.EDGE:
            assert C.chain(a, b).lazy % P == a * b % P
            for c in (0, 1, P - 1, C.M64, C.M64 - (a * b & C.M64), 1 << 32):
                assert C.chain(a, b, c).lazy % P == (a * b + c) % P


def test_chain_on_all_half_word_operands_reaches_every_class_and_corner():
    w, count = C.witnesses()          # runs `chain` (and its assertions) over all 16^4 pairs
    assert sum(count[k] for k in C.CLASSES) == 16 ** 4
    for k in C.CLASSES + C.CORNERS:
        assert count[k] > 0 and w[k], "no witness of %r" % (k,)
    ch = C.chain(0xFFFFFFFF00000002, 0xFFFFFFFFFFFFFFFF)
    assert ch.corner == C.CORNERS[0] and ch.cy == 1 and ch.borrow == 1


def test_chain_on_random_pairs():
    rng = np.random.default_rng(20)
    n = 400000
    a = rng.integers(0, 1 << 64, n, dtype=np.uint64).tolist()
    b = rng.integers(0, 1 << 64, n, dtype=np.uint64).tolist()
    c = rng.integers(0, 1 << 64, n, dtype=np.uint64).tolist()
    cys = 0
    for i in range(n):
        cys += C.chain(a[i], b[i]).cy
        if i % 8 == 0:
            C.chain(a[i], b[i], c[i])
    assert cys > n // 100   # the cross carry is no rare path: a few per cent of uniform products


def test_chain_on_borrow_operands():
    rng = np.random.default_rng(21)
    ts = [int(t) for t in rng.integers(1, 1 << 64, 3000, dtype=np.uint64)] + [int(rng.integers(1 << 16, 1 << 31)) << 32 for _ in range(500)]
    seen = carry = 0
    for t in ts:
        x = R.borrow_operand(t, rng, canonical=False)
        if x is None:
            continue
        ch = C.chain(x, t)
        assert ch.borrow and R.mul_paths(x, t).borrow
        assert ch.lazy == R.mul_paths(x, t).lazy       # the same lazy word as the two-argument reduction, not only the same class
        seen += 1
        carry += ch.cy
    assert seen > 2000 and carry > 0, (seen, carry)


def test_witness_array_covers_every_class_and_corner_in_every_pattern():
    A, B, masks = C.witness_array()
    assert len(masks) == (len(C.CLASSES) + len(C.CORNERS)) * len(R.PATTERNS)
    for key, name, off, mask in masks:
        planted = 0
        for i in np.nonzero(mask)[0]:
            ch = C.chain(A[off + i], B[off + i])
            assert (ch[:4] == key) if key in C.CLASSES else (ch.corner == key), (key, name, int(i))
            planted += 1
        assert planted >= 16, (key, name)   # lane0 of 1024 lanes: one per wave


def test_poseidon_and_hash_inputs_are_carry_and_borrow_witnesses():
    st, wit = C.poseidon_carry_borrow_states(R.patterns(256)["alternate"], 30)
    assert len(wit) == 128 * 12
    rows, wit2 = C.hash_carry_borrow_rows(9, R.patterns(256)["lane0"], 31)
    assert rows.shape == (256, 9) and len(wit2) == 4 * 9
    for x, y in wit + wit2:
        ch = C.chain(x, y)
        assert ch.cy == 1 and ch.borrow == 1 and R.mul_paths(x, y).borrow
    assert (st < np.uint64(P)).all() and (rows < np.uint64(P)).all()
