"""The paired forms of the radix-16 NTT passes on the device. `field_reduce2` runs `gl::reduce128_lazy2` (two borrow chains issued
alternately, ONE test of their ORed masks) on 128-bit words of every class in slot A against every class in slot B under every lane
pattern (tests/ntt_pair_cases.py; counted on the CPU by tests/test_gl_reduce_pairs.py). Then where the pairs are inlined: forward and
inverse transforms at the sizes that take each shape of pass, the coset LDE (the products on load) and inputs whose first-stage
PAIR of shifts repairs in its first chain only, its second only, and both."""
import os

import numpy as np
import pytest

import ntt_pair_cases as NP
import oracle_lib as O
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


def test_field_reduce2_every_class_against_every_class_in_every_lane_pattern(prover):
    la, ha, lb, hb, want_a, want_b, blocks = NP.reduce_array()
    got_a, got_b = prover.field_reduce2(la, ha, lb, hb)
    where = {off // NP.N: (ka, kb, name) for ka, kb, name, off in blocks}
    for slot, got, want, lo, hi in (("A", got_a, want_a, la, ha), ("B", got_b, want_b, lb, hb)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(slot, where[int(i) // NP.N], int(i) % NP.N, hex(int(lo[i])), hex(int(hi[i])), int(got[i]), int(want[i])) for i in bad[:5]]


def test_field_reduce2_odd_count_and_swapped_slots(prover):
    """a count that is no multiple of the wave or the workgroup, and the slots exchanged: each chain's repair stays its own"""
    la, ha, lb, hb, want_a, want_b, _ = NP.reduce_array()
    n = 5 * NP.N + 37
    got_b, got_a = prover.field_reduce2(lb[:n], hb[:n], la[:n], ha[:n])
    assert (got_a == want_a[:n]).all() and (got_b == want_b[:n]).all()


# 2^12: one whole-tile pass; 2^13: L = 7 + 6; 2^16: the one-round column pass and a HALF row pass; 2^17: L = 5; 2^20: 8 + 12
@pytest.mark.parametrize("log_n", [12, 13, 16, 17, 20])
def test_forward_and_inverse_transforms_of_two_columns(prover, log_n):
    x = O.splitmix64_felts(0x9A1B5 + log_n, 2 << log_n).reshape(2, -1)
    got = prover.ntt(x)
    for c in range(2):
        assert (got[c] == O.ntt(x[c])).all(), ("forward", log_n, c)
    got = prover.intt(x)          # the inverse carries the 1 / n scale of the last pass
    for c in range(2):
        assert (got[c] == O.intt(x[c])).all(), ("inverse", log_n, c)


@pytest.mark.parametrize("log_n", [12, 16])
def test_rate_2_coset_lde(prover, log_n):
    """2^12: two coset transforms through the pre-scale table; 2^16: the zero-padded transform with the coset powers on load"""
    c = O.splitmix64_felts(0x1DE + log_n, 2 << log_n).reshape(2, -1)
    got = prover.lde(c, 1, shift=7, bitrev=True)
    for b in range(2):
        assert (got[b] == O.bit_reverse(O.coset_lde(c[b], 1, 7))).all(), (log_n, b)


def base_mask(log_n, pattern):
    """the lane pattern over the first 256 of the n / 16 base indices (one workgroup's threads of the first tile)"""
    m = np.zeros(1 << (log_n - 4), bool)
    m[:256] = R.patterns(256)[pattern]
    return m


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [12, 16])
def test_repair_in_the_first_chain_the_second_and_both_of_a_first_stage_pair(prover, log_n, inverse):
    oracle = O.intt if inverse else O.ntt
    run = prover.intt if inverse else prover.ntt
    for combo in NP.COMBOS:
        for pattern in ("every_lane", "lane63", "alternate"):
            x, wit = NP.ntt16_pair_input(log_n, inverse, combo, base_mask(log_n, pattern), 31 * log_n + inverse)
            assert wit and all((R.pow2_paths(da, Ka).borrow, R.pow2_paths(db, Kb).borrow) == combo for da, Ka, db, Kb in wit[:8])
            assert (run(x) == oracle(x)).all(), (log_n, inverse, combo, pattern)
    # the K < 64 pairs, whose second shift (K <= 32) cannot repair: the first chain alone, planted in the eighths of their first shifts
    n = 1 << log_n
    for eighth in (1, 4):
        Ka = R.W16_SHIFT[inverse][eighth] % 96
        assert any(ra - 8 == eighth and rb is not None and Kb <= 32 for ra, _, rb, Kb in NP.stage_plan(inverse, 3)) and 33 <= Ka < 64
        mask = np.zeros(n // 2, bool)
        mask[eighth * (n >> 4):eighth * (n >> 4) + 256] = R.patterns(256)["alternate"]
        x, wit = R.ntt16_borrow_input(log_n, inverse, mask, 77 + eighth)
        assert len(wit) == 128 and all(K == Ka and R.pow2_paths(d, K).borrow for d, K in wit)
        assert (run(x) == oracle(x)).all(), (log_n, inverse, eighth)
