"""The 2^-32 paths of csrc/gl.h driven inside every kernel family, device against oracle / Python integers, bit for bit.

`reduce128_lazy` repairs the borrow of `lo - w3` behind a wave-uniform branch in hand-written `asm`, and `canon` matters only for
results below 2^32 - 1: uniform data meets either about once in 2^32 products, so tests on random inputs say nothing about how the
inlined code was scheduled in Poseidon, the Merkle kernels, the NTT passes, FRI, the AIR interpreter, the cubic inversion, the
prefix sum and the Z kernel. Every case here builds inputs whose FIRST multiplication in that kernel has operands known on the host
(tests/rare_paths.py), asserts with the classifier that they take the path, and compares the whole output; borrow cases are repeated
over the lane patterns (all lanes of a wave, one, half, none). The `build_*` functions make the inputs and touch no GPU:
tests/test_rare_paths.py calls them all on the CPU.

Not reached: a Merkle DIGEST below 2^32 - 1. The capacity of the sponge is fixed at zero, and the permutation cannot be inverted
under that constraint, so hash outputs cannot be chosen (the raw permutation's can, and are). Also `7 * bb` in ext_mul cannot
borrow at all (the product is below 2^67: w3 = 0); its wrap and its canon are what the small-result cases reach.

How far the planted operands go. Only the FIRST multiplication of a kernel has operands the host knows; everything after it sees
what a hash or a butterfly made of them, which is uniform again.
- Merkle: the leaf kernels meet the borrow in every absorbed block of a hashed leaf, and every level form meets it in the first tree
  level, over leaves of four elements that are their own digests (test_merkle_forms_borrow_in_the_first_level). The second and later
  levels of a fused or cooperative launch read digests and are not planted (under lane_leaf_fuse1..3 they are further trips of the
  `#pragma unroll 1` loop of fused_levels whose first trip is).
- NTT / LDE: the first stage of the first pass (mul_pow2<K> in the radix-16 kernels, the twiddle product in the generic one), the
  coset pre-scale and the LDE pre-scale meet planted borrows. The template instances that run as second and third pass (row passes
  of 6 or 7 bits) and the inter-pass / T3 twiddle products multiply transformed data, so they run here without a planted borrow;
  their launch labels are asserted, their rare paths are not reached.

Checked against two deliberately wrong builds of the library (never committed): with the borrow repair removed every borrow case
below fails; with `canon` made the identity the small-output cases whose value reaches HBM through a product or through Poseidon's
final canon fail. Where the last operation is gl::add (FRI fold and combine, the point evaluation's block sum, the forward
butterflies) the `(s < a) | (s >= P)` repair of the addition absorbs one non-canonical addend, so those small-result cases pin the
addition's repair, not canon."""
import numpy as np
import pytest

import air_programs as A
import oracle_lib as O
import rare_paths as R
import test_gpu_merkle_forms as MF
import test_gpu_ntt_forms as NF

pytestmark = pytest.mark.gpu
P = O.P
LANES = 1024                      # four workgroups of 256: the last pattern plants one wave in two of them
INVERSE, BITREV_OUT, COSET = NF.INVERSE, NF.BITREV_OUT, NF.COSET
NTT_SIZES = (10, 12, 13, 16, 21)   # one below 2^12 (generic kernel), then the radix-16 plans 12, 7+6, 4+12, 7+7+7
SHIFT = 7


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def assert_borrows(wit, least=1):
    assert len(wit) >= least, "only %d planted products" % len(wit)
    assert all(R.mul_paths(a, b).borrow for a, b in wit)


def assert_pow2_borrows(wit, least=1):
    assert len(wit) >= least
    assert all(R.pow2_paths(d, K).borrow for d, K in wit)
    return {K for _, K in wit}


def mask_for(pattern, n=LANES):
    return R.patterns(n)[pattern]


# ---- Poseidon: the raw permutation -----------------------------------------------------------------------------------------
def build_poseidon_borrow(pattern):
    st, wit = R.poseidon_borrow_states(mask_for(pattern), 1000 + R.PATTERNS.index(pattern))
    assert_borrows(wit, 12 * 16)
    return st


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_poseidon_permute_borrow_in_the_first_sbox(prover, pattern):
    st = build_poseidon_borrow(pattern)
    assert (prover.poseidon_permute(st) == O.permute_many(st).reshape(-1, 12)).all()


CANON_STATES = 128


def build_poseidon_canon():
    return R.poseidon_canon_targets(CANON_STATES, 2000)


def test_poseidon_permute_outputs_below_2_32(prover):
    """outputs chosen through the inverse permutation: 0 .. 12 elements of a state below 2^32 - 1 (tests/test_rare_paths.py counts how
    many of them the device formulas hold as value + p before the final canon)"""
    X, T = build_poseidon_canon()
    got = prover.poseidon_permute(X)
    assert (got == T).all(), np.nonzero(got != T)


def build_poseidon_partial():
    X = R.poseidon_partial_round_inputs()
    return np.concatenate([X] * 3 + [O.splitmix64_felts(77, 12 * 44).reshape(-1, 12)])   # a few waves, special rows in several lanes


def test_poseidon_partial_rounds_at_extreme_limbs(prover):
    """the double-precision layers entered with all-ones limbs and the sign patterns that maximise the ab / b components"""
    X = build_poseidon_partial()
    assert (prover.poseidon_permute(X) == O.permute_many(X).reshape(-1, 12)).all()


# ---- hash_no_pad, two_to_one, every Merkle form -------------------------------------------------------------------------------
HASH_LENGTHS = [5, 8, 9, 20]


def build_hash_no_pad(length, pattern):
    cols, wit = R.leaf_columns(length, mask_for(pattern), 3000 + length)
    assert_borrows(wit, 16 * length)
    return np.ascontiguousarray(cols.T)


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("length", HASH_LENGTHS)
def test_hash_no_pad_borrow_in_every_absorbed_block(prover, length, pattern):
    x = build_hash_no_pad(length, pattern)
    got = prover.hash_no_pad(x)
    want = np.array([O.hash_no_pad(r) for r in x], dtype=np.uint64)
    assert (got == want).all()


def build_two_to_one(pattern):
    cols, wit = R.leaf_columns(8, mask_for(pattern), 3100)
    assert_borrows(wit, 16 * 8)
    return np.ascontiguousarray(cols[:4].T), np.ascontiguousarray(cols[4:].T)


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_two_to_one_borrow(prover, pattern):
    l, r = build_two_to_one(pattern)
    got = prover.two_to_one(l, r)
    want = np.array([O.two_to_one(a, b) for a, b in zip(l, r)], dtype=np.uint64)
    assert (got == want).all()


def merkle_shape_for(row):
    """the first shape of test_gpu_merkle_forms.SHAPES with hashed leaves on which the planner runs the row's form"""
    opts, label = MF.ROWS[row]
    for log_n, leaf_len, cap_h in MF.SHAPES:
        if leaf_len > 4 and log_n >= 9 and MF.merkle_plan(1 << log_n, leaf_len, 1, cap_h, opts)[label] > 0:
            return log_n, leaf_len, cap_h
    raise AssertionError("no shape runs the form of row " + row)


def build_merkle(row, pattern):
    log_n, leaf_len, cap_h = merkle_shape_for(row)
    cols, wit = R.leaf_columns(leaf_len, mask_for(pattern, 1 << log_n), 3200 + log_n + leaf_len)
    assert_borrows(wit, leaf_len)
    return cols, cap_h


@pytest.mark.parametrize("row", sorted(MF.ROWS))
def test_merkle_forms_borrow_in_the_leaf_hash(row):
    opts, label = MF.ROWS[row]
    p = MF.forced(opts)
    try:
        for pattern in R.PATTERNS:
            cols, cap_h = build_merkle(row, pattern)
            want_cap, want_dig = O.merkle_tree_cols(cols, cap_h, want_digests=True)
            out = {}
            launches = MF.measured(p, lambda: out.update(r=p.merkle_cols(cols, cap_h, want_digests=True)))
            cap, dig = out["r"]
            assert (cap == want_cap).all(), (row, pattern)
            assert (dig == want_dig).all(), ("digests", row, pattern)
            assert launches == MF.merkle_plan(cols.shape[1], cols.shape[0], 1, cap_h, opts) and launches[label] > 0, (row, dict(launches))
    finally:
        p.close()


# The rows above reach the LEAF kernels only: what a level kernel reads there is a digest, uniform data. Leaves of four elements are
# their own digests, so with them the kernel that hashes the first level takes its whole state from the host (R.level_columns) and no
# kernel below it multiplies at all. row -> (label of the launch that hashes the leaves' parents, levels that launch fuses on top /
# walks): merkle_level is k_level, which no row names and lane_leaf_fuse0 runs; under lane_leaf_fuse1..3 the first level is the
# fused part of the leaf kernel. The levels above the first read digests again, in every form.
LEVEL_ROWS = {"lane_leaf_fuse0": ("merkle_level", 0), "coop_level": ("merkle_level_coop", 0)}
for _f in range(1, 4):
    LEVEL_ROWS["lane_leaf_fuse%d" % _f] = ("leaf_hash_cols", _f)
    LEVEL_ROWS["level_fuse%d" % _f] = ("merkle_level_fused", _f)
for _k in range(1, 6):
    LEVEL_ROWS["coop_levels_fused%d" % _k] = ("merkle_levels_coop", _k)


def first_level_launch(n, cap_h, opts):
    """(label, depth) of the launch that hashes the parents of n unhashed leaves: the first step of cityprover.hip merkle_cols_batch /
    merkle_levels, from the helpers of test_gpu_merkle_forms (its merkle_plan counts launches and does not say which comes first)"""
    o = dict(MF.DEFAULTS, **opts)
    cap_n, np_ = 1 << cap_h, n // 2
    f = MF.leaf_fuse_eff(n, 1, cap_h, opts)
    if f:
        return "leaf_hash_cols", f
    if np_ <= o["COOP_MAX"] and o["COOP_FUSE"] >= 1:
        levels = 0
        while levels < min(o["COOP_FUSE"], MF.COOP_MAX_FUSED) and (n >> levels) > cap_n:
            levels += 1
        return "merkle_levels_coop", levels
    fuse = 0 if np_ == cap_n else MF.fusable_levels(np_, cap_n, MF._clip3(o["MERKLE_LEVEL_FUSE"]))
    while fuse > 0 and (np_ >> fuse) < o["COOP_MAX"]:
        fuse -= 1
    if fuse:
        return "merkle_level_fused", fuse
    return ("merkle_level_coop" if np_ <= o["COOP_MAX"] else "merkle_level"), 0


def merkle_level_shape_for(row):
    """the first shape of test_gpu_merkle_forms.SHAPES with unhashed leaves whose first level is computed by the row's level form"""
    opts, _ = MF.ROWS[row]
    for log_n, leaf_len, cap_h in MF.SHAPES:
        if leaf_len == 4 and log_n >= 9 and first_level_launch(1 << log_n, cap_h, opts) == LEVEL_ROWS[row]:
            plan = MF.merkle_plan(1 << log_n, leaf_len, 1, cap_h, opts)
            assert plan[LEVEL_ROWS[row][0]] > 0 and plan["leaf_hash_cols_coop"] == 0, (row, dict(plan))
            return log_n, cap_h
    raise AssertionError("no shape runs the level form of row " + row)


def build_merkle_level(row, pattern):
    log_n, cap_h = merkle_level_shape_for(row)
    cols, wit = R.level_columns(mask_for(pattern, 1 << (log_n - 1)), 3300 + log_n)
    assert_borrows(wit, 8)
    return cols, cap_h


@pytest.mark.parametrize("row", sorted(LEVEL_ROWS))
def test_merkle_forms_borrow_in_the_first_level(row):
    """the borrow inside k_level, k_level_fused<1..3>, the fused part of k_leaf_hash_cols<., 1..3>, k_level_coop and k_levels_coop: the
    pattern lies over the parent index, which is the lane in the lane-per-parent kernels and the 12-lane group in the cooperative ones
    (there lanes 0..7 of a group borrow and 8..11 do not)"""
    opts, _ = MF.ROWS[row]
    label = LEVEL_ROWS[row][0]
    p = MF.forced(opts)
    try:
        for pattern in R.PATTERNS:
            cols, cap_h = build_merkle_level(row, pattern)
            want_cap, want_dig = O.merkle_tree_cols(cols, cap_h, want_digests=True)
            out = {}
            launches = MF.measured(p, lambda: out.update(r=p.merkle_cols(cols, cap_h, want_digests=True)))
            cap, dig = out["r"]
            assert (cap == want_cap).all(), (row, pattern)
            assert (dig == want_dig).all(), ("digests", row, pattern)
            assert launches == MF.merkle_plan(cols.shape[1], cols.shape[0], 1, cap_h, opts) and launches[label] > 0, (row, dict(launches))
    finally:
        p.close()


# ---- NTT / LDE --------------------------------------------------------------------------------------------------------------
def window_mask(pattern, log_n, half):
    """the pattern on the first LANES lanes of each eighth of the first half (the eight shift twiddles of the first stage), or of
    the first 4096 indices: the planted positions stay a few thousand at 2^21"""
    n = 1 << log_n
    if not half:
        m = np.zeros(n, bool)
        w = min(n, 4096)
        m[:w] = mask_for(pattern, w)
        return m
    m = np.zeros(n // 2, bool)
    block = n >> 4
    w = min(block, LANES)
    for e in range(8):
        m[e * block:e * block + w] = mask_for(pattern, w)
    return m


def build_ntt_borrow(log_n, pattern):
    """[(flags, shift, x, wanted shifts or None)]: forward and inverse first-stage cases, and the coset pre-scale"""
    seed = 4000 + 16 * log_n + R.PATTERNS.index(pattern)
    cases = []
    first = NF.dif_plan(log_n)[0][1]
    if first.startswith("ntt16"):
        for inv in (False, True):
            x, wit = R.ntt16_borrow_input(log_n, inv, window_mask(pattern, log_n, True), seed + inv)
            ks = assert_pow2_borrows(wit, 5)
            assert ks == set(R.BORROW_SHIFTS), ks
            cases.append((INVERSE if inv else 0, 0, x))
    else:
        for inv in (False, True):
            x, wit = R.twiddle_borrow_input(log_n, R.root_of_unity(log_n, inv), mask_for(pattern, 1 << (log_n - 1)), seed + inv, second_half_zero=True)
            assert_borrows(wit, 4)
            cases.append((INVERSE if inv else 0, 0, x))
    x, wit = R.twiddle_borrow_input(log_n, SHIFT, window_mask(pattern, log_n, False), seed + 2)
    assert_borrows(wit, 8)
    cases.append((COSET, SHIFT, x))
    return cases


def oracle_ntt(x, flags, shift):
    if flags & COSET:
        return O.coset_lde(x, 0, shift)
    return O.intt(x) if flags & INVERSE else O.ntt(x)


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("log_n", NTT_SIZES)
def test_ntt_borrow_in_the_first_stage_and_the_coset_prescale(prover, log_n, pattern):
    for flags, shift, x in build_ntt_borrow(log_n, pattern):
        got, launches = NF.call(prover, prover.ntt, x, flags=flags, shift=shift)
        assert (got == oracle_ntt(x, flags, shift)).all(), (log_n, flags, pattern)
        assert launches == NF.ntt_plan(log_n, flags), (log_n, flags, dict(launches))


def build_ntt_borrow_legacy(pattern):
    """2^13 under CITYPROVER_NTT_V1: the generic kernel as a column pass over the top 7 index bits (ntt_dif_pass_cols), whose first
    butterfly multiplies x[i] - x[i + n/2] by omega_128^(i >> 6)"""
    log_n = 13
    L = NF.dif_plan(log_n, v1=True)[0][0]
    cases = []
    for inv in (False, True):
        x, wit = R.twiddle_borrow_input(log_n, R.root_of_unity(L, inv), window_mask(pattern, log_n, False)[:1 << (log_n - 1)],
                                        4900 + inv, q=log_n - L, second_half_zero=True)
        assert_borrows(wit, 8)
        cases.append((INVERSE if inv else 0, x))
    return cases


def legacy_generic_kernel_checks(prover):
    """the body of test_ntt_borrow_in_the_legacy_generic_column_pass: runs in a process started with CITYPROVER_NTT_V1 set"""
    for pattern in R.PATTERNS:
        for flags, x in build_ntt_borrow_legacy(pattern):
            got, launches = NF.call(prover, prover.ntt, x, flags=flags)
            assert (got == oracle_ntt(x, flags, 0)).all(), (flags, pattern)
            assert launches == NF.ntt_plan(13, flags, v1=True) and launches["ntt_dif_pass_cols"] == 1, dict(launches)
    Y = build_ntt_small(13)
    assert (prover.ntt(O.intt(Y)) == Y).all() and (prover.intt(O.ntt(Y)) == Y).all()


CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import cityprover
import test_gpu_rare_paths as T
p = cityprover.Prover(0)
T.legacy_generic_kernel_checks(p)
p.close()
print("rare paths v1 ok")
"""


def test_ntt_borrow_in_the_legacy_generic_column_pass():
    import os
    import subprocess
    import sys
    env = dict(os.environ, CITYPROVER_NTT_V1="1")
    code = CHILD.format(tests=os.path.join(NF.ROOT, "tests"), pkg=os.path.join(NF.ROOT, "city-rollup_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0 and "rare paths v1 ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


LDE_SMALL_CASES = [(12, 3, True), (12, 3, False), (10, 2, False), (13, 1, True)]      # (log_n, rate, bitrev)
LDE_PRESCALE_SMALL_CASES = [(12, 3, True), (10, 2, False), (13, 1, True)]
LDE_PRESCALE_BORROW_CASE = (12, 3, True)


def ntt_labels_covered():
    """the launch labels of the plans the NTT / LDE cases of this module assert their launches against, from the same size and case
    lists the tests are parametrised with (a label here is a kernel that ran, not one whose first product was planted: see the module
    docstring)"""
    labels = set(NF.ntt_plan(13, 0, v1=True)) | set(NF.ntt_plan(13, INVERSE, v1=True))      # legacy_generic_kernel_checks
    for log_n in NTT_SIZES:                                                                  # build_ntt_borrow: 0, INVERSE, COSET
        for flags in (0, INVERSE, COSET):
            labels |= set(NF.ntt_plan(log_n, flags))
    for log_n, rate, bitrev in LDE_SMALL_CASES + LDE_PRESCALE_SMALL_CASES + [LDE_PRESCALE_BORROW_CASE]:
        labels |= set(NF.lde_plan(log_n, rate, bitrev))
    return labels


def build_ntt_small(log_n):
    return R.small_values(1 << log_n, 5000 + log_n)


@pytest.mark.parametrize("log_n", NTT_SIZES)
def test_ntt_outputs_below_2_32(prover, log_n):
    """every output element below 2^32 - 1, forward and inverse, natural and bit-reversed order"""
    Y = build_ntt_small(log_n)
    x = O.intt(Y)
    assert (prover.ntt(x) == Y).all()
    assert (prover.ntt(x, flags=BITREV_OUT) == O.bit_reverse(Y)).all()
    x = O.ntt(Y)
    assert (prover.intt(x) == Y).all()
    assert (prover.ntt(x, flags=INVERSE | BITREV_OUT) == O.bit_reverse(Y)).all()


def build_lde_small(log_n, rate):
    """coefficients whose evaluations on the coset SHIFT <omega_n> (every 2^rate-th point of the LDE) are all below 2^32 - 1"""
    Y = R.small_values(1 << log_n, 5100 + log_n)
    c = O.intt(Y)
    si = pow(SHIFT, P - 2, P)
    out, t = np.zeros_like(c), 1
    for i in range(c.size):
        out[i] = int(c[i]) * t % P
        t = t * si % P
    return out, Y


@pytest.mark.parametrize("log_n,rate,bitrev", LDE_SMALL_CASES)
def test_lde_with_one_coset_block_below_2_32(prover, log_n, rate, bitrev):
    c, Y = build_lde_small(log_n, rate)
    want = O.coset_lde(c, rate, SHIFT)
    assert (want[::1 << rate] == Y).all()
    got, launches = NF.call(prover, prover.lde, c, rate, shift=SHIFT, bitrev=bitrev)
    got = got.reshape(-1)
    assert (got == (O.bit_reverse(want) if bitrev else want)).all()
    assert launches == NF.lde_plan(log_n, rate, bitrev), dict(launches)


def build_lde_small_prescale(log_n):
    """coefficients whose product with shift^j — the first thing either LDE path computes — is below 2^32 - 1 for every j"""
    y = R.small_values(1 << log_n, 5300 + log_n)
    c, t = np.zeros_like(y), 1
    for j in range(y.size):
        c[j] = R.small_product_operand(t, int(y[j]))
        t = t * SHIFT % P
    return c


@pytest.mark.parametrize("log_n,rate,bitrev", LDE_PRESCALE_SMALL_CASES)
def test_lde_prescale_products_below_2_32(prover, log_n, rate, bitrev):
    """forward transforms end in additions and subtractions, whose own repairs make the result canonical: there the canon that
    matters is the one of the pre-scale product, which the butterflies take as a canonical operand"""
    c = build_lde_small_prescale(log_n)
    want = O.coset_lde(c, rate, SHIFT)
    got, launches = NF.call(prover, prover.lde, c, rate, shift=SHIFT, bitrev=bitrev)
    assert (got.reshape(-1) == (O.bit_reverse(want) if bitrev else want)).all()
    assert launches == NF.lde_plan(log_n, rate, bitrev), dict(launches)


def build_lde_prescale_borrow(pattern):
    log_n = LDE_PRESCALE_BORROW_CASE[0]
    x, wit = R.twiddle_borrow_input(log_n, SHIFT, window_mask(pattern, log_n, False), 5200)
    assert_borrows(wit, 16)
    return x


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_lde_prescale_borrow(prover, pattern):
    """the LDE at 2^12 multiplies coefficient j by (shift omega_N^r)^j from a table; block r = 0 is shift^j"""
    log_n, rate, bitrev = LDE_PRESCALE_BORROW_CASE
    x = build_lde_prescale_borrow(pattern)
    got, launches = NF.call(prover, prover.lde, x, rate, shift=SHIFT, bitrev=bitrev)
    assert (got.reshape(-1) == O.bit_reverse(O.coset_lde(x, rate, SHIFT))).all()
    assert launches == NF.lde_plan(log_n, rate, bitrev)


# ---- FRI combine / fold, evaluation at a point ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("odd_beta", [False, True])
@pytest.mark.parametrize("arity_bits", [1, 3])
def test_fri_fold_borrow_in_each_base_product(prover, arity_bits, odd_beta, pattern):
    import cityprover
    c, beta, wit = R.fri_fold_input(LANES, arity_bits, mask_for(pattern), 6000 + arity_bits, odd_beta)
    assert_borrows(wit, 16)
    assert (cityprover.fri_fold(prover, c, arity_bits, beta) == R.fri_fold_py(c, arity_bits, beta)).all()


def test_fri_fold_components_below_2_32(prover):
    import cityprover
    c, beta, want = R.fri_fold_small_input(LANES, 2, 6100)
    assert (R.fri_fold_py(c, 2, beta) == want).all() and (want < R.SMALL).all()
    assert (cityprover.fri_fold(prover, c, 2, beta) == want).all()


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("k", [3, 19])
def test_fri_combine_borrow(prover, k, pattern):
    import cityprover
    f, alpha, ap, wit = R.fri_combine_input(k, mask_for(pattern), 6200 + k)
    assert_borrows(wit, 16)
    assert (cityprover.fri_combine(prover, f, alpha) == R.fri_combine_py(f, ap)).all()


def test_fri_combine_components_below_2_32(prover):
    import cityprover
    f, alpha, ap, want = R.fri_combine_small_input(11, LANES, 6300)
    assert (R.fri_combine_py(f, ap) == want).all() and (want < R.SMALL).all()
    assert (cityprover.fri_combine(prover, f, alpha) == want).all()


def build_eval_ext(pattern):
    """cp_batch_eval_ext: sum_j c[j] z^j with the powers z^j made on the device; k_eval_at_point multiplies c[j] by the two components
    of z^j, thread t of a polynomial's workgroup taking j = t, t + 256, ...: the pattern over the coefficient index j is a pattern over
    the lanes (and its workgroup period a period over the trips of that loop). z = (u << 32, odd); z^j is computed on the host, and
    under the mask, j >= 1, coefficient j of polynomial q borrows against component (j + q) & 1 of z^j."""
    k, db = 8, 10
    rng = np.random.default_rng(6400)
    polys = rng.integers(0, P, (k, 1 << db), dtype=np.uint64)
    z = (int(rng.integers(1 << 20, 1 << 31)) << 32, int(rng.integers(1, P, dtype=np.uint64)) | 1)
    zp, wit = (1, 0), []
    m = mask_for(pattern, 1 << db)
    for j in range(1, 1 << db):
        zp = R.ext_mul_py(zp, z)
        if not m[j]:
            continue
        for p_ in range(k):
            t = zp[(j + p_) & 1]
            v = R.borrow_operand(t, rng)
            if v is not None:
                polys[p_, j] = v
                wit.append((v, t))
    assert_borrows(wit, 8 * 8)
    return polys, np.array(z, dtype=np.uint64), db


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_batch_eval_ext_borrow(prover, pattern):
    import cityprover
    coeffs, z, db = build_eval_ext(pattern)
    g = cityprover.PolyBatch(prover, coeffs, 1, 2, from_coeffs=True)
    o = O.Batch(coeffs, 1, 2, True)
    try:
        assert (g.eval_ext(z) == o.eval_ext(z)).all()
    finally:
        g.close()
        o.close()


def build_eval_ext_small():
    """polynomials whose value at z has both components below 2^32 - 1: c[1] settles .b (z.b != 0), then c[0] settles .a"""
    k, db = 8, 10
    rng = np.random.default_rng(6500)
    polys = rng.integers(0, P, (k, 1 << db), dtype=np.uint64)
    z = (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    polys[:, :2] = 0
    rest, zp = [(0, 0)] * k, (1, 0)
    for j in range(1 << db):
        rest = [((a + int(c) * zp[0]) % P, (b + int(c) * zp[1]) % P) for (a, b), c in zip(rest, polys[:, j])]
        zp = R.ext_mul_py(zp, z)
    want = np.stack([R.small_values(k, 6501), R.small_values(k, 6502)[::-1]], axis=1)
    binv = pow(z[1], P - 2, P)
    for q in range(k):
        c1 = (int(want[q, 1]) - rest[q][1]) * binv % P
        polys[q, 1] = c1
        polys[q, 0] = (int(want[q, 0]) - rest[q][0] - c1 * z[0]) % P
    return polys, np.array(z, dtype=np.uint64), want


def test_batch_eval_ext_components_below_2_32(prover):
    import cityprover
    coeffs, z, want = build_eval_ext_small()
    assert (want < R.SMALL).all()
    g = cityprover.PolyBatch(prover, coeffs, 1, 2, from_coeffs=True)
    o = O.Batch(coeffs, 1, 2, True)
    try:
        assert (o.eval_ext(z) == want).all()
        assert (g.eval_ext(z) == want).all()
    finally:
        g.close()
        o.close()


# ---- the AIR interpreter ---------------------------------------------------------------------------------------------------------
def product_program(kind):
    if kind == A.MAP:
        b = A.Builder(A.MAP, 2, n_out_columns=1)
        b.store(0, b.mul(b.local(0), b.local(1)))
    else:
        b = A.Builder(A.CONSTRAINTS, 2)
        b.assert_zero(b.mul(b.local(0), b.local(1)))
    return b


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_air_map_product_borrow(prover, pattern):
    import cityprover
    cols, wit = R.product_columns(mask_for(pattern), 7000)
    assert_borrows(wit, 16)
    b = product_program(A.MAP)
    g, o = b.gpu(prover), b.oracle()
    try:
        assert (cityprover.air_map(prover, g, cols) == o.map(cols)).all()
    finally:
        g.close()


def test_air_map_products_below_2_32(prover):
    import cityprover
    cols, want = R.small_product_columns(LANES, 7100)
    b = product_program(A.MAP)
    g = b.gpu(prover)
    try:
        assert (cityprover.air_map(prover, g, cols)[0] == want).all()
    finally:
        g.close()


def build_quotient_constants():
    """two constant columns: a degree-0 polynomial has a constant LDE, so MUL(local(0), local(1)) borrows at every point of the coset
    (every lane of every wave: the one pattern constant columns allow)"""
    rng = np.random.default_rng(7200)
    out = []
    for t in (int(rng.integers(1 << 20, 1 << 31)) << 32, int(rng.integers(0, P, dtype=np.uint64)) | 1):
        v = R.borrow_operand(t, rng)
        assert_borrows([(v, t)])
        out.append((v, t))
    return out


@pytest.mark.parametrize("db,rb,q", [(8, 1, 1), (10, 2, 2)])
def test_air_quotient_commit_product_of_constant_columns_borrows(prover, db, rb, q):
    import cityprover
    for v, t in build_quotient_constants():
        trace = np.empty((2, 1 << db), np.uint64)
        trace[0], trace[1] = v, t
        alphas = np.array([3, P - 5], dtype=np.uint64)
        b = product_program(A.CONSTRAINTS)
        G, Ob = cityprover.PolyBatch(prover, trace, rb, 2), O.Batch(trace, rb, 2)
        g, o = b.gpu(prover), b.oracle()
        try:
            want = O.air_quotient(o, [Ob], q, alphas)
            Q = cityprover.air_quotient_commit(prover, g, [G], q, alphas)
            try:
                assert (Q.coeffs() == want).all()
            finally:
                Q.close()
        finally:
            g.close()
            G.close()
            Ob.close()


# ---- cubic inversion, prefix sum, Z / partial products -----------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_cubic_batch_inverse_borrow_against_the_modulus(prover, pattern):
    import cityprover
    for m, cols, wit in R.cubic_inverse_input(9, mask_for(pattern), 8000):
        assert_borrows(wit, 16 * 9)
        assert (cityprover.cubic_batch_inverse(prover, m, cols) == O.cubic_batch_inverse(m, cols)).all(), m


@pytest.mark.parametrize("n", [1 << 10, 100000])
def test_prefix_sum_across_p_and_below_2_32(prover, n):
    """gl::add's repair `(s < a) | (s >= P)`: the wrapped sum and the unwrapped sum in [p, 2^64), thousands of each, and running sums
    below 2^32 - 1"""
    import cityprover
    cols, (wrapped, only_ge_p, small) = R.prefix_sum_columns(n, 8100)
    assert wrapped > n // 4 and only_ge_p > n // 4 and small > n // 4, (wrapped, only_ge_p, small)
    for ex in (False, True):
        assert (cityprover.column_prefix_sum(prover, cols, ex) == O.column_prefix_sum(cols, ex)).all(), ex


ZS_SHAPE = dict(db=10, R=20, W=24, chunk=4, nc=2, B=2)


def build_zs(pattern):
    s = ZS_SHAPE
    out = R.zs_input(s["db"], s["R"], s["W"], s["nc"], s["B"], mask_for(pattern, 1 << s["db"]), 8200)
    assert_borrows(out[-1], 8)
    return out


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_zs_partial_products_beta_sigma_borrows_on_whole_rows(prover, pattern):
    import cityprover as cp
    s = ZS_SHAPE
    db, Rr, Wn, chunk, nc, B = (s[k] for k in ("db", "R", "W", "chunk", "nc", "B"))
    wires, sig, betas, gammas, _ = build_zs(pattern)
    npp = (Rr + chunk - 1) // chunk - 1
    kw = dict(degree_bits=db, num_constants=3, num_routed_wires=Rr, num_wires=Wn, num_challenges=nc, num_partial_products=npp,
              quotient_degree_factor=chunk, rate_bits=3, cap_height=2, pow_bits=4, num_query_rounds=3, arity_bits=(2,))
    sh = cp.standard_recursion_shape(**kw)
    osh = O.standard_shape(degree_bits=db, num_wires=Wn, num_routed=Rr, num_constants=3, num_challenges=nc, num_partial_products=npp,
                           quotient_degree_factor=chunk, rate_bits=3, cap_height=2, pow_bits=4, num_query_rounds=3, arity_bits=(2,))
    n = 1 << db
    k_is = [pow(7, j, P) for j in range(Rr)]
    cs = np.concatenate([O.splitmix64_felts(51, 3 * n).reshape(3, n), sig])
    circ = cp.Circuit(prover, sh, [1, 0, 0, 0], cs)
    dw, dout = prover.to_device(wires), prover.alloc(B * nc * (1 + npp) * n)
    try:
        cp.zs_partial_products_dev(prover, [circ] * B, dw.ptr, betas, gammas, dout.ptr)
        got = dout.download().reshape(B, nc * (1 + npp), n)
        for b in range(B):
            assert (got[b] == O.zs_partial_products(osh, wires[b], sig, k_is, betas[b], gammas[b])).all(), b
    finally:
        dw.free()
        dout.free()
        circ.close()
