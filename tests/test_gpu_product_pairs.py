"""The paired product of csrc/gl.h (`mul_lazy2`) on the device: two product chains issued alternately with ONE test of their ORed borrow
masks. `field_mul2` runs it on every class and corner of the product chain in slot A against every one in slot B under every lane
pattern (tests/product_pairs.py; counted on the CPU by tests/test_gl_product_pairs.py); then where it is inlined: the paired S-boxes
of a permutation's first round with (repair, none), (none, repair) and (both) on the partners of each pair, the sponge, and one
Merkle tree in the lane-per-leaf and the twelve-lane forms."""
import os

import numpy as np
import pytest

import oracle_lib as O
import product_chain as C
import product_pairs as PP
import rare_paths as R

pytestmark = pytest.mark.gpu
P = O.P


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


def test_field_mul2_every_class_against_every_class_in_every_lane_pattern(prover):
    A, B, C_, D, blocks = PP.pair_array()
    want_ab, want_cd = PP.pair_products()
    got_ab, got_cd = prover.field_mul2(A, B, C_, D)
    where = {off // PP.N: (ka, kb, name) for ka, kb, name, off, _ in blocks}
    for slot, got, want, x, y in (("A", got_ab, want_ab, A, B), ("B", got_cd, want_cd, C_, D)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(slot, where[int(i) // PP.N], int(i) % PP.N, hex(int(x[i])), hex(int(y[i])), int(got[i]), int(want[i])) for i in bad[:5]]


def test_field_mul2_odd_count_and_swapped_slots(prover):
    """a count that is no multiple of the wave or the workgroup, and the slots exchanged: each chain's repair stays its own"""
    A, B, C_, D, _ = PP.pair_array()
    want_ab, want_cd = PP.pair_products()
    n = 5 * PP.N + 37
    got_cd, got_ab = prover.field_mul2(C_[:n], D[:n], A[:n], B[:n])
    assert (got_ab == want_ab[:n]).all() and (got_cd == want_cd[:n]).all()


def test_poseidon_permute_repairs_on_either_partner_of_every_first_round_pair(prover):
    st, what = PP.poseidon_pair_states()
    assert len(what) == 256
    assert (prover.poseidon_permute(st) == O.permute_many(st).reshape(-1, 12)).all()


@pytest.mark.parametrize("length", [9, 135])
def test_hash_no_pad_on_256_rows(prover, length):
    """every absorbed element of every second row is a (cy = 1, repaired) first squaring; in every fourth row only the even positions
    are, so a pair of S-boxes has one partner that repairs and one that does not"""
    x, wit = C.hash_carry_borrow_rows(length, R.patterns(256)["alternate"], 600 + length)
    assert len(wit) == 128 * length
    fresh = O.splitmix64_felts(700 + length, 256 * length).reshape(256, length)
    x[::4, 1::2] = fresh[::4, 1::2]
    want = np.array([O.hash_no_pad(r) for r in x], dtype=np.uint64)
    assert (prover.hash_no_pad(x) == want).all()


_tree = []


def tree():
    if not _tree:
        cols = O.splitmix64_felts(0x5B0C5, 135 << 9).reshape(135, -1)
        _tree.append((cols,) + tuple(O.merkle_tree_cols(cols, 0, want_digests=True)))
    return _tree[0]


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("lane", [True, False])
def test_merkle_tree_of_512_leaves_in_every_digest(fuse, lane):
    """lane: the lane-per-leaf leaf hash and the lane-per-parent level kernel (paired S-boxes); else the twelve-lane kernels the size
    gets by default (the single S-box with its paired x^3, x^4)"""
    import cityprover
    cols, want_cap, want_dig = tree()
    p = cityprover.Prover(0)
    try:
        p.set_option("MERKLE_FUSE", fuse)
        if lane:
            p.set_option("COOP_LEAF_MAX", 0)
            p.set_option("COOP_MAX", 0)
        cap, dig = p.merkle_cols(cols, 0, want_digests=True)
        assert (cap == want_cap).all() and (dig == want_dig).all()
    finally:
        p.close()
