"""tests/rare_paths.py checked on the CPU: the path classifier against the device formulas instantiated on the host (hostsim), the
inverse Poseidon permutation against the oracle, the operand constructors, and every input builder of
tests/test_gpu_rare_paths.py (shapes and witnesses fail here, without a GPU)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import rare_paths as R
import test_gpu_rare_paths as T

P = O.P
M = (1 << 64) - 1
p64 = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def hs():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("hostsim"))
    lib.hs_mul_paths.restype = ctypes.c_int
    lib.hs_mul_paths.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.hs_mul_pow2.restype = ctypes.c_uint64
    lib.hs_mul_pow2.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.hs_poseidon_permute_lazy.argtypes = [p64, ctypes.c_size_t]
    lib.hs_poseidon_permute.argtypes = [p64, ctypes.c_size_t]
    return lib


def bits(paths):
    return int(paths.borrow) | int(paths.fold_wrap) << 1 | int(paths.lazy_ge_p) << 2


def field_mul_operands():
    """the operand set of tests/test_gpu_parity.py::test_field_mul_every_carry_and_borrow_corner (without its 600 000 random pairs)"""
    rng = np.random.default_rng(11)
    edge = [0, 1, 2, 3, P - 1, P - 2, P, P + 1, M, M - 1, 0xFFFFFFFF, 0x100000000, 0x100000001, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001,
            1 << 63, (1 << 63) + 1, 0x7FFFFFFF80000000, 0x8000000080000000, 0xFFFFFFFFFFFF0000, 1 << 48, 3 << 48, 1 << 32, 1 << 33]
    a = [x for x in edge for _ in edge]
    b = [y for _ in edge for y in edge]
    for _ in range(2000):
        u, k = int(rng.integers(1 << 16, 1 << 32)), int(rng.integers(1 << 16, 1 << 32))
        a.append(u << 32)
        b.append(k << 32)
    for _ in range(2000):
        aa = int(rng.integers(1 << 62, 1 << 64, dtype=np.uint64)) | 1
        t = int(rng.integers(1, 1 << 20))
        a.append(aa)
        b.append((t * pow(aa, -1, 1 << 64)) & M)
    hi_vals = [0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0xFFFF0000, 1]
    for a1 in hi_vals:
        for a0 in hi_vals:
            for b1 in hi_vals:
                for b0 in hi_vals:
                    a.append((a1 << 32) | a0)
                    b.append((b1 << 32) | b0)
    return a, b


def test_classifier_equals_hostsim(hs):
    a, b = field_mul_operands()
    rng = np.random.default_rng(12)
    ra = rng.integers(0, 1 << 64, 100000, dtype=np.uint64)
    rb = rng.integers(0, 1 << 64, 100000, dtype=np.uint64)
    small = [(R.small_product_operand(int(t) | 1, int(v)), int(t) | 1) for t, v in zip(ra[:3000], rng.integers(0, R.SMALL, 3000))]
    seen = [0, 0, 0]
    for x, y in list(zip(a, b)) + [(int(x), int(y)) for x, y in zip(ra, rb)] + small:   # small: products below 2^32 - 1, the ones canon is for
        want = bits(R.mul_paths(x, y))
        assert hs.hs_mul_paths(x, y) == want, (hex(x), hex(y))
        for k in range(3):
            seen[k] += want >> k & 1
    assert min(seen) > 1000, seen   # each of the three paths was compared on more than a thousand pairs


def test_pow2_classifier(hs):
    """pow2_paths is consistent with mul_pow2 on the host (the lazy value it derives is the product), the borrow needs K >= 33, and
    pow2_borrow_operand borrows by construction"""
    rng = np.random.default_rng(13)
    for K in (1, 12, 24, 32, 33, 36, 48, 60, 72, 84):
        for x in [int(v) for v in rng.integers(0, P, 200, dtype=np.uint64)] + [1, P - 1, 1 << 63, 0xFFFFFFFF00000000]:
            pp = R.pow2_paths(x, K)
            if K < 64:
                assert pp.lazy % P == hs.hs_mul_pow2(x, K)
            assert not (pp.borrow and K < 33)
        if K >= 33:
            for _ in range(200):
                d = R.pow2_borrow_operand(K, rng)
                assert d < P and R.pow2_paths(d, K).borrow
                assert hs.hs_mul_pow2(d, K) == (d << K) % P


def test_seven_times_bb_cannot_borrow():
    rng = np.random.default_rng(14)
    for bb in [P - 1, M, 1 << 63] + [int(v) for v in rng.integers(0, 1 << 64, 2000, dtype=np.uint64)]:
        assert not R.mul_paths(bb, 7).borrow
    assert R.mul_paths(M, 7).fold_wrap


def test_constructors_borrow_by_construction():
    rng = np.random.default_rng(15)
    ts = [int(v) for v in rng.integers(1 << 32, P, 300, dtype=np.uint64)]
    ts += [int(v) | 1 for v in rng.integers(1 << 32, P, 300, dtype=np.uint64)]
    ts += [int(v) << 32 for v in rng.integers(1 << 16, 1 << 31, 300)]
    ts += [int(v) << s for s in (1, 7, 13) for v in rng.integers(1 << 40, 1 << 50, 50)]     # even, few trailing zeros
    ts += [int(v) << s for s in (20, 31, 33, 40) for v in rng.integers(1 << 20, 1 << 23, 50)]
    ts += [R.root_of_unity(k) for k in range(3, 25)] + [pow(7, i, P) for i in range(16, 60)]   # 7^i below 2^44 leaves w3 next to nothing
    for t in ts:
        x = R.borrow_operand(t, rng)
        assert x is not None and x < P and R.mul_paths(x, t).borrow, hex(t)
    for t in (0, 1, 7, 0xFFFFFFFF):
        assert R.borrow_operand(t, rng) is None      # w3 == 0 whenever the low word is small
    for t in ts[:200]:
        for v in (0, 1, R.SMALL - 1, int(rng.integers(0, R.SMALL))):
            x = R.small_product_operand(t, v)
            assert x < P and x * t % P == v


def test_patterns():
    pat = R.patterns(1024)
    assert tuple(pat) == R.PATTERNS and len(pat) == 5
    per_wave = {k: m.reshape(-1, 64).sum(axis=1).tolist() for k, m in pat.items()}
    assert per_wave["every_lane"] == [64] * 16 and per_wave["lane0"] == [1] * 16 and per_wave["lane63"] == [1] * 16
    assert pat["lane0"][0] and pat["lane63"][63] and per_wave["alternate"] == [32] * 16
    assert per_wave["one_wave_per_other_workgroup"] == [0, 64, 0, 0, 0, 0, 0, 0] * 2


def test_inverse_permutation_is_the_inverse_in_both_orders():
    st = O.splitmix64_felts(4242, 12 * 200).reshape(-1, 12)
    edge = np.array([0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 1 << 63, (1 << 63) + 1,
                     0x7FFFFFFF80000000], np.uint64)
    st = np.concatenate([st, edge[None], np.roll(edge, 5)[None], np.zeros((1, 12), np.uint64), np.full((1, 12), P - 1, np.uint64)])
    for s in st:
        fwd = O.permute(s)
        assert [int(v) for v in fwd] == R.permute(s)                       # the Python forward permutation is the oracle's
        assert R.inverse_permute(fwd) == [int(v) for v in s]
        assert [int(v) for v in O.permute(np.array(R.inverse_permute(s), np.uint64))] == [int(v) for v in s]
    for u in R.PARTIAL_TARGETS[:6]:
        assert R.sbox_outputs_of_round3(R.input_for_sbox_outputs_of_round3(u)) == u


def test_targeted_small_outputs_are_held_as_value_plus_p(hs):
    """Observed for the committed seed (N = 128 states, 12 N = 1536 output elements): 1380 elements are targeted below 2^32 - 1 and
    all 1380 leave the last layer as value + p (zero leaves it as p), so the final canon decides every one of them; of the 156
    other elements none does. The last layer ends in fold_top with a non-zero top word, which lands on value + p for such values."""
    X, Tg = T.build_poseidon_canon()
    lazy = X.copy()
    hs.hs_poseidon_permute_lazy(lazy.ctypes.data_as(p64), lazy.shape[0])
    assert all(int(a) % P == int(b) for a, b in zip(lazy.ravel(), Tg.ravel()))
    small = Tg < R.SMALL
    need = lazy >= np.uint64(P)
    assert int((need & small).sum()) >= 1000
    got = X.copy()
    hs.hs_poseidon_permute(got.ctypes.data_as(p64), got.shape[0])
    assert (got == Tg).all()


def test_partial_round_targets_run_the_device_formulas_bit_exact(hs):
    X = T.build_poseidon_partial()
    got = X.copy()
    hs.hs_poseidon_permute(got.ctypes.data_as(p64), got.shape[0])
    assert (got == O.permute_many(X).reshape(-1, 12)).all()
    for x, u in zip(X, R.PARTIAL_TARGETS):
        assert R.sbox_outputs_of_round3(x) == u


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_every_gpu_case_builder(pattern):
    """the builders assert their own witnesses; here also shapes, canonical inputs and the Python references"""
    st = T.build_poseidon_borrow(pattern)
    assert st.shape == (T.LANES, 12) and (st < P).all()
    for length in T.HASH_LENGTHS:
        x = T.build_hash_no_pad(length, pattern)
        assert x.shape == (T.LANES, length) and (x < P).all()
    l, r = T.build_two_to_one(pattern)
    assert l.shape == r.shape == (T.LANES, 4) and (l < P).all() and (r < P).all()
    for row in sorted(T.MF.ROWS):
        cols, cap_h = T.build_merkle(row, pattern)
        assert cols.shape[0] > 4 and (cols < P).all()
    for row in sorted(T.LEVEL_ROWS):
        cols, cap_h = T.build_merkle_level(row, pattern)
        assert cols.shape[0] == 4 and (cols < P).all()
    x = T.build_lde_prescale_borrow(pattern)
    assert x.shape == (1 << T.LDE_PRESCALE_BORROW_CASE[0],) and (x < P).all()
    for log_n in T.NTT_SIZES:
        for flags, shift, x in T.build_ntt_borrow(log_n, pattern):
            assert x.shape == (1 << log_n,) and (x < P).all()
    for flags, x in T.build_ntt_borrow_legacy(pattern):
        assert x.shape == (1 << 13,) and (x < P).all()
    for odd in (False, True):
        c, beta, wit = R.fri_fold_input(T.LANES, 3, T.mask_for(pattern), 6003, odd)
        T.assert_borrows(wit, 16)
        assert (c < P).all() and (beta < P).all()
    f, alpha, ap, wit = R.fri_combine_input(19, T.mask_for(pattern), 6219)
    T.assert_borrows(wit, 16)
    assert (f < P).all() and ap[1] == (int(alpha[0]), int(alpha[1]))
    coeffs, z, db = T.build_eval_ext(pattern)
    assert (coeffs < P).all() and (z < P).all()
    cols, wit = R.product_columns(T.mask_for(pattern), 7000)
    assert (cols < P).all()
    for m, cols, wit in R.cubic_inverse_input(9, T.mask_for(pattern), 8000):
        T.assert_borrows(wit, 16 * 9)
        assert (cols < P).all() and m[0] < P and m[1] < P
    wires, sig, betas, gammas, wit = T.build_zs(pattern)
    assert (sig < P).all() and (betas < P).all()


def test_small_output_builders():
    X, Tg = T.build_poseidon_canon()
    counts = sorted(int((t < R.SMALL).sum()) for t in Tg)
    assert counts[0] == 0 and counts[-1] == 12 and set(range(13)) <= set(counts)
    assert all(v in Tg for v in (0, 1, R.SMALL - 1))
    for log_n in T.NTT_SIZES:
        Y = T.build_ntt_small(log_n)
        assert Y.shape == (1 << log_n,) and (Y < R.SMALL).all()
        if log_n <= 16:
            assert (O.ntt(O.intt(Y)) == Y).all()
    coeffs, z, want = T.build_eval_ext_small()
    assert (coeffs < P).all() and (want < R.SMALL).all()
    ob = O.Batch(coeffs, 1, 2, True)
    try:
        assert (ob.eval_ext(z) == want).all()
    finally:
        ob.close()
    c, Y = T.build_lde_small(10, 2)
    assert (O.coset_lde(c, 2, T.SHIFT)[::4] == Y).all() and (c < P).all()
    c = T.build_lde_small_prescale(10)
    assert (c < P).all() and all(int(c[j]) * pow(T.SHIFT, j, P) % P < R.SMALL for j in range(0, 1024, 37))
    c, beta, want = R.fri_fold_small_input(64, 2, 6100)
    assert (R.fri_fold_py(c, 2, beta) == want).all() and (want < R.SMALL).all()
    f, alpha, ap, want = R.fri_combine_small_input(11, 64, 6300)
    assert (R.fri_combine_py(f, ap) == want).all() and (want < R.SMALL).all()
    cols, want = R.small_product_columns(64, 7100)
    assert all(int(a) * int(b) % P == int(w) for a, b, w in zip(cols[0], cols[1], want))
    cols, (wrapped, only_ge_p, small) = R.prefix_sum_columns(1 << 10, 8100)
    assert (cols < P).all() and min(wrapped, only_ge_p, small) > 256
    assert (O.column_prefix_sum(cols)[0, 1::2] < R.SMALL).all()
    assert len(T.build_quotient_constants()) == 2


def test_ntt_cases_cover_every_launch_label():
    assert T.ntt_labels_covered() == set(T.NF.LABELS)


def test_every_level_form_has_a_shape_whose_first_level_it_hashes():
    """every Merkle row but coop_leaf (a leaf form: unhashed leaves never run it) has a level case, on a shape of the planner test whose
    leaves are their own digests, and the launch that hashes the first level there is the row's own at its full depth"""
    assert set(T.LEVEL_ROWS) == set(T.MF.ROWS) - {"coop_leaf"}
    for row, (label, depth) in T.LEVEL_ROWS.items():
        opts, row_label = T.MF.ROWS[row]
        assert label == row_label or row == "lane_leaf_fuse0"
        log_n, cap_h = T.merkle_level_shape_for(row)
        assert (log_n, 4, cap_h) in T.MF.SHAPES
        assert depth == max([0] + [v for k, v in opts.items() if k in ("MERKLE_FUSE", "MERKLE_LEVEL_FUSE", "COOP_FUSE")])
    cols, wit = R.level_columns(R.patterns(8)["every_lane"], 1)
    for j in range(8):       # the state the level kernel permutes: leaf 2j | leaf 2j + 1, each position c against its own round constant
        state = [int(v) for v in cols[:, 2 * j]] + [int(v) for v in cols[:, 2 * j + 1]]
        assert all((state[c] + R.RC[c]) % (1 << 32) == 0 and state[c] + R.RC[c] < P for c in range(8))
