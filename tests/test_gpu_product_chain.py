"""The carry-aware product chain of csrc/gl.h on the device: the carry-out of the product's third multiply-add stays in its SGPR pair
and enters the borrow chain of the reduction as a carry-in. Every class of (cy, low-word borrow, 64-bit borrow, fold wrap) and the
two corners that exist only because of the carry-in (tests/product_chain.py, counted on the CPU by tests/test_gl_product_chain.py)
under every lane pattern through `field_mul`; then the product where it is inlined: the first S-box of a permutation and of a
sponge, and both radix-16 NTT plans with their lazy power walks."""
import numpy as np
import pytest

import oracle_lib as O
import product_chain as C
import rare_paths as R

pytestmark = pytest.mark.gpu
P = O.P
SHIFT = 7
COSET = 4   # cityprover.NTT_COSET (asserted below)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    assert cityprover.NTT_COSET == COSET
    p = cityprover.Prover(0)
    yield p
    p.close()


def test_field_mul_every_class_and_corner_in_every_lane_pattern(prover):
    A, B, masks = C.witness_array()
    got = prover.field_mul(A, B)
    want = np.array([int(x) * int(y) % P for x, y in zip(A.tolist(), B.tolist())], dtype=np.uint64)
    bad = np.nonzero(got != want)[0]
    where = {off // 1024: (key, name) for key, name, off, _ in masks}
    assert bad.size == 0, [(where[int(i) // 1024], int(i) % 1024, hex(int(A[i])), hex(int(B[i])), int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_poseidon_permute_carry_and_borrow_in_the_first_sbox(prover, pattern):
    st, wit = C.poseidon_carry_borrow_states(R.patterns(256)[pattern], 100 + R.PATTERNS.index(pattern))
    assert len(wit) >= 12 and all(C.chain(x, y).cy and C.chain(x, y).borrow for x, y in wit)
    assert (prover.poseidon_permute(st) == O.permute_many(st).reshape(-1, 12)).all()


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_hash_no_pad_of_nine_carry_and_borrow_in_both_blocks(prover, pattern):
    x, wit = C.hash_carry_borrow_rows(9, R.patterns(256)[pattern], 200 + R.PATTERNS.index(pattern))
    assert len(wit) >= 9 and all(C.chain(a, b).cy and C.chain(a, b).borrow for a, b in wit)
    want = np.array([O.hash_no_pad(r) for r in x], dtype=np.uint64)
    assert (prover.hash_no_pad(x) == want).all()


def ntt_inputs(log_n):
    """forward transform: borrowing mul_pow2 operands in the first stage; coset transform: borrowing pre-scale products"""
    n = 1 << log_n
    m = np.zeros(n // 2, bool)
    for e in range(8):
        m[e * (n >> 4):e * (n >> 4) + 128] = R.patterns(128)["alternate"]
    x, wit = R.ntt16_borrow_input(log_n, False, m, 300 + log_n)
    assert {K for _, K in wit} == set(R.BORROW_SHIFTS) and all(R.pow2_paths(d, K).borrow for d, K in wit)
    m = np.zeros(n, bool)
    m[:1024] = R.patterns(1024)["one_wave_per_other_workgroup"] | R.patterns(1024)["lane63"]
    y, wit = R.twiddle_borrow_input(log_n, SHIFT, m, 400 + log_n)
    assert len(wit) >= 64 and all(C.chain(a, b).borrow for a, b in wit) and any(C.chain(a, b).cy for a, b in wit)
    return x, y


@pytest.mark.parametrize("log_n", [12, 16])   # one radix-16 pass; two passes: half-tile exchange, inter-pass power walk, staged store
def test_forward_ntt_one_pass_and_two_passes(prover, log_n):
    x, y = ntt_inputs(log_n)
    assert (prover.ntt(x) == O.ntt(x)).all()
    assert (prover.ntt(y, flags=COSET, shift=SHIFT) == O.coset_lde(y, 0, SHIFT)).all()
    u = O.splitmix64_felts(500 + log_n, 1 << log_n)       # every T3 / inter-pass power on uniform data
    assert (prover.ntt(u) == O.ntt(u)).all()
