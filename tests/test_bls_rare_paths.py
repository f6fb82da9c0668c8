"""tests/bls_rare_paths.py checked on the CPU: the restatements against the device formulas instantiated on the host (hostsim),
the constructions against the restatements, a false positive of the "same x?" filter against a LOOSE accumulator (the order
inside a bucket is fixed only here), mul_small over its extremes, and every input builder of tests/test_gpu_bls_rare_paths.py:
witnesses and shares of planted positions fail here, without a GPU."""
import ctypes

import numpy as np
import pytest

import bls_rare_paths as B
import oracle_lib as O
import test_gpu_bls_rare_paths as T

u32p = ctypes.POINTER(ctypes.c_uint32)
MIN_SHARE = 15 / 16          # at most 1 in 16 planted positions of a case may fall back to random data


@pytest.fixture(scope="module")
def hs():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("hostsim"))
    for name in ("hs_bls_g1_loose_step", "hs_bls_g2_loose_step", "hs_bls_g1_loose_out", "hs_bls_g2_loose_out", "hs_bls_lz_k", "hs_bls_lz_maybe_zero"):
        getattr(lib, name).restype = ctypes.c_int
    return lib


def w32(vals):
    return np.array(list(vals), dtype=np.uint32)


def ptr(a):
    return a.ctypes.data_as(u32p)


def fr_raw(hs, op, a, b):
    out = np.zeros(B.FR_NL, np.uint32)
    x = w32(B.limbs(a, B.FR_NL)) if op != 3 else w32([(a >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    y = w32(B.limbs(b, B.FR_NL))
    hs.hs_bls_fr_raw(op, ptr(x), ptr(y), ptr(out))
    return B.value(out)


def fp_raw(hs, op, al, bl):
    out = np.zeros(B.FP_NL, np.uint32)
    x, y = w32(al), w32(bl)
    hs.hs_bls_fp_raw(op, ptr(x), ptr(y), ptr(out))
    return tuple(int(v) for v in out)


def assert_fr_witnesses(hs, pairs):
    """every pair subtracts by the restatement, and the real fr_mul returns the subtracted value (it does not when its final
    fr_cond_sub is taken out)"""
    for a, b in pairs:
        t = B.fr_t(a, b)
        assert 0 < a < B.R and 0 < b < B.R and B.R <= t < 2 * B.R, (hex(a), hex(b))
        assert fr_raw(hs, 0, a, b) == t - B.R, (hex(a), hex(b))


# ---- 1. the product scan ------------------------------------------------------------------------------------------------------------
def test_product_scan_restatement_equals_the_real_code(hs):
    """mont_t (integers), scan (limb by limb) and fr_mul / fp_mul / lz_mul / lz_sqr of the headers agree; random products of F_r
    never subtract here (about 2^-27 each), those of F_p do (p / 2^392 = 2^-11.3)"""
    rng = np.random.default_rng(1)
    subs = [0]
    for _ in range(300):
        a, b = B.rand_below(rng, B.R), B.rand_below(rng, B.R)
        t = B.fr_t(a, b)
        assert B.value(B.scan(B.limbs(a, B.FR_NL), B.limbs(b, B.FR_NL), B.R, B.FR_NL)[0]) == t
        assert fr_raw(hs, 0, a, b) == B.fr_mul(a, b) == a * b * B.RR_INV % B.R
        subs[0] += t >= B.R
        a, b = B.rand_below(rng, B.P), B.rand_below(rng, B.P)
        al, bl = B.limbs(a, B.FP_NL), B.limbs(b, B.FP_NL)
        t = B.fp_t(a, b)
        assert B.value(B.scan(al, bl, B.P, B.FP_NL)[0]) == t
        assert B.value(fp_raw(hs, 0, al, bl)) == B.fp_mul(a, b) and fp_raw(hs, 1, al, bl) == B.lz_mul(al, bl) == B.limbs(t, B.FP_NL)
        assert fp_raw(hs, 2, al, al) == B.lz_sqr(al) and B.value(fp_raw(hs, 3, al, al)) == B.fp_mul(a, a)
    assert subs[0] == 0
    found = 0
    while found < 20:                     # F_p products that do subtract: a search of a few thousand pairs each
        a, b = B.rand_below(rng, B.P), B.rand_below(rng, B.P)
        if B.fp_t(a, b) >= B.P:
            found += 1
            al, bl = B.limbs(a, B.FP_NL), B.limbs(b, B.FP_NL)
            assert B.value(fp_raw(hs, 0, al, bl)) == B.fp_t(a, b) - B.P == a * b * B.RP_INV % B.P and fp_raw(hs, 1, al, bl) == B.limbs(B.fp_t(a, b), B.FP_NL)
    for a in (0, 1, B.R - 1, B.R - 2, B.ONE_R, B.R2_R):
        for b in (0, 1, B.R - 1, B.ONE_R, B.R2_R):
            assert fr_raw(hs, 0, a, b) == B.fr_mul(a, b)


def test_columns_at_the_edge_of_the_64_bit_bound(hs):
    """bls12_381.h: operands with a b < R p and limbs below 2^29 keep a column of the scan below 2^62.3. Fed here: every limb
    2^29 - 1 up to the value bound (the unnormalised sums lz_add_nc hands to lz_mul), saturated normalised limbs, and the
    saturated-limb coordinates of the GPU cases."""
    rng = np.random.default_rng(2)
    top = 0
    ops = []
    full = (B.LM,) * (B.FP_NL - 1)
    for t in (0, 1, 0x1A010):
        ops.append(full + (t,))                                  # saturated, normalised, below p
    wide = [(1 << 29) - 1] * B.FP_NL                              # limbs below 2^29, value trimmed to stay below 32 p
    wide[-1] = (32 * B.P >> (B.LB * (B.FP_NL - 1))) - 2
    ops.append(tuple(wide))
    ops += [B.limbs(B.mont_x(q), B.FP_NL) for q in B.g1_saturated(4)]
    ops += [B.limbs(B.rand_below(rng, B.P), B.FP_NL) for _ in range(4)]
    for al in ops:
        for bl in ops:
            if B.value(al) * B.value(bl) >= B.RADIX_P * B.P:
                continue
            got, col = B.scan(al, bl, B.P, B.FP_NL)
            top = max(top, col)
            assert col < 2 ** 62.3
            assert got == B.lz_mul(al, bl) == fp_raw(hs, 1, al, bl) and B.value(got) < 2 * B.P
            assert B.value(fp_raw(hs, 0, al, bl)) == B.value(al) * B.value(bl) * B.RP_INV % B.P
        assert fp_raw(hs, 2, al, al) == B.lz_sqr(al)
    assert top > 2 ** 61.5, "the operands above reach the neighbourhood of the bound"


def test_loose_primitives_equal_the_real_code(hs):
    rng = np.random.default_rng(3)
    out = np.zeros(B.FP_NL, np.uint32)
    for K in (2, 4, 6, 8, 10, 12, 16, 18, 22):
        for _ in range(60):
            a = B.limbs(B.rand_below(rng, 22 * B.P), B.FP_NL)
            b = B.limbs(B.rand_below(rng, K * B.P + 1), B.FP_NL)
            if rng.random() < 0.3:                                # unnormalised operands, as lz_add_nc leaves them
                a = B.lz_add_nc(a, B.limbs(B.rand_below(rng, 2 * B.P), B.FP_NL))
                b2 = B.limbs(B.rand_below(rng, K * B.P // 2), B.FP_NL)
                b = B.lz_add_nc(b2, b2)
            x, y = w32(a), w32(b)
            assert hs.hs_bls_lz_k(0, K, ptr(x), ptr(y), ptr(out)) == 0
            got = tuple(int(v) for v in out)
            assert got == B.lz_sub(K, a, b) and B.value(got) == B.value(a) + K * B.P - B.value(b)
            for v in (B.rand_below(rng, 2 * K * B.P), K * B.P, K * B.P - 1, K * B.P + 1):
                a = B.limbs(v, B.FP_NL)
                x = w32(a)
                assert hs.hs_bls_lz_k(1, K, ptr(x), ptr(x), ptr(out)) == 0
                assert tuple(int(t) for t in out) == B.lz_weak(K, a) == B.limbs(v - K * B.P if v >= K * B.P else v, B.FP_NL)
    for _ in range(500):
        a = B.limbs(B.rand_below(rng, 32 * B.P), B.FP_NL)
        b = B.limbs(B.rand_below(rng, 2 * B.P), B.FP_NL)
        assert fp_raw(hs, 4, a, b) == B.lz_add_nc(a, b)
        x = w32(a)
        assert hs.hs_bls_lz_maybe_zero(ptr(x)) == int(B.lz_maybe_zero(a))
    for k in range(32):
        assert B.lz_maybe_zero(B.limbs(k * B.P, B.FP_NL))
    assert not B.lz_maybe_zero(B.limbs(32 * B.P, B.FP_NL))


# ---- 2. F_r operands ------------------------------------------------------------------------------------------------------------------
def test_plant_fr_builds_operands_that_subtract(hs):
    rng = np.random.default_rng(4)
    pairs, failed = [], 0
    for b in [B.rand_below(rng, B.R) for _ in range(300)] + [B.R - 1, B.R - 2, B.R2_R, B.fr_mont(7), B.fr_mont(pow(7, -1, B.R))]:
        a = B.plant_fr(b, rng)
        failed += a is None
        if a is not None:
            pairs.append((a, b))
    assert failed <= len(pairs) // 16
    assert_fr_witnesses(hs, pairs)
    for _ in range(50):                       # the load conversion of a canonical input
        a = B.plant_fr_load(rng)
        assert B.fr_subtracts(a, B.R2_R) and fr_raw(hs, 3, a, 0) == a * B.RADIX_R % B.R == B.fr_t(a, B.R2_R) - B.R
        x = B.plant_fr_value(B.fr_mont(12345), rng)
        assert B.fr_subtracts(B.fr_mont(x), B.fr_mont(12345))
    # b = 1 (fr_to_canonical, the right side of k_check) needs a = 0
    assert B.plant_fr(1, rng) is None and B.plant_fr(0, rng) is None
    # values in [2^254, r) are drawn by the random fill
    assert any(v >> 254 for v in B.fr_random(rng, 64)) and all(v < B.R for v in B.fr_random(rng, 4096))


# ---- 3. mul_small -----------------------------------------------------------------------------------------------------------------------
def small_raw(hs, w, c):
    out = np.zeros(B.FR_NL, np.uint32)
    x = w32(B.limbs(w, B.FR_NL))
    hs.hs_r1cs_mul_small(ptr(x), ctypes.c_uint32(c), ptr(out))
    return B.value(out)


def test_mul_small_over_its_extremes(hs):
    """The grid of the edge operands, constructed pairs that need exactly one subtraction and pairs that need none with a
    remainder just below r, all against c w mod r. The second conditional subtraction is not reachable: with R1 = floor(r / 2^224)
    and g = 2^224 (R1 + 1) - r < 2^224, t / r - T1 / (R1 + 1) < t g / (r (r + g)) + 1 / (R1 + 1) < 2^28 * 2^224 / 2^254.8 + 2^-30
    < 0.14, so t - q' r < 1.14 r < 2 r for every w < r and c < 2^28; the restatement agrees over every operand below (the largest
    remainder it sees is printed). The second fr_cond_sub of the code is left alone."""
    rng = np.random.default_rng(5)
    sat = [B.value((B.LM,) * 9 + (t,)) for t in (0, 1, 0x73EC)] + [B.value((0,) * 9 + (0x73ED,)), B.R - (1 << 224), (B.R >> 224) << 224]
    ws = [0, 1, B.R - 1, B.R - 2] + [w for w in sat if w < B.R]
    cs = [2, 3, 1 << 27, (1 << 28) - 2, (1 << 28) - 1]
    seen = [0, 0, 0]
    worst = 0

    def one(w, c):
        nonlocal worst
        m = B.mul_small(w, c)
        assert m.result == w * c % B.R and m.q_est <= m.q and small_raw(hs, w, c) == m.result, (hex(w), c)
        seen[m.n_sub] += 1
        worst = max(worst, (w * c - m.q_est * B.R) * 1000 // B.R)
        return m

    for w in ws:
        for c in cs:
            one(w, c)
    one_sub, near = B.mul_small_pairs(rng, 400)
    assert all(one(w, c).n_sub == 1 for w, c in one_sub)
    for w, c in near:
        m = one(w, c)
        assert m.n_sub == 0 and B.R - m.result <= c
    for _ in range(20000):                                        # skewed towards w = r - 1, c = 2^28 - 1: where the estimate is worst
        one(B.R - 1 - B.rand_below(rng, 1 << int(rng.integers(1, 250))), (1 << 28) - 1 - B.rand_below(rng, 1 << int(rng.integers(1, 27))))
    print("mul_small subtractions 0/1/2:", seen, "largest remainder before them: %.3f r" % (worst / 1000))
    assert seen[1] >= 400 and seen[2] == 0 and worst < 1140


# ---- 4. the loose mixed addition ------------------------------------------------------------------------------------------------------
def acc_words(acc):
    return w32([x for c in acc for f in B.components(c) for x in f])


def xy_words(pt):
    two = isinstance(pt[0], tuple)
    coords = [c for xy in pt for c in (xy if two else [xy])]
    return w32([(c >> (32 * i)) & 0xFFFFFFFF for c in coords for i in range(12)])


def real_chain(hs, points):
    """the chain through the real xyzz_add_mixed_loose, step by step against the restatement (limbs and way); returns the affine
    result of the real code and the restatement's steps"""
    two = isinstance(points[0][0], tuple)
    step = hs.hs_bls_g2_loose_step if two else hs.hs_bls_g1_loose_step
    acc = B.xyzz_inf(two)
    n = 8 if two else 4
    steps = []
    for pt in points:
        st = B.xyzz_add_mixed_loose(acc, B.mont_point(pt))
        a, q, out = acc_words(acc), xy_words(pt), np.zeros(n * B.FP_NL, np.uint32)
        way = step(ptr(a), ptr(q), ptr(out))
        assert way >= 0 and B.WAYS[way] == st.way
        assert out.tolist() == acc_words(st.acc).tolist()
        assert B.within_bounds(st.acc) or B.lf_is_zero(st.acc[2])
        steps.append(st)
        acc = st.acc
    a, xy = acc_words(acc), np.zeros(48 if two else 24, np.uint32)
    inf = (hs.hs_bls_g2_loose_out if two else hs.hs_bls_g1_loose_out)(ptr(a), ptr(xy))
    val = lambda k: sum(int(v) << (32 * i) for i, v in enumerate(xy[12 * k:12 * k + 12]))
    if inf:
        return None, steps
    return (((val(0), val(1)), (val(2), val(3))) if two else (val(0), val(1))), steps


def oracle_sum(points):
    add = O.bls_g2_add if isinstance(points[0][0], tuple) else O.bls_g1_add
    s = None
    for q in points:
        s = add(s, q)
    return s


def test_false_positive_pairs_families_and_saturated_points(hs):
    """every point builder: on the curve (by the oracle too), the filter passes in both orders, the G2 mixed cases are what they
    say, families are pairwise false positives, and the real addition equals the restatement and the oracle's sum"""
    rng = np.random.default_rng(6)
    for _ in range(10):
        a, b = B.g1_false_positive_pair(rng)
        assert O.bls_g1_on_curve(a) and O.bls_g1_on_curve(b) and a[0] != b[0]
        for pts in ([a, b], [b, a]):
            got, steps = real_chain(hs, pts)
            assert steps[1].way == "false_positive" and got == oracle_sum(pts)
    for mode in ("both", "c0_zero", "c0_alias_c1_equal"):
        for _ in range(6):
            a, b = B.g2_false_positive_pair(rng, mode)
            assert O.bls_g2_on_curve(a) and O.bls_g2_on_curve(b) and a[0] != b[0]
            for pts in ([a, b], [b, a]):
                got, steps = real_chain(hs, pts)
                st = steps[1]
                assert got == oracle_sum(pts)
                if mode == "c0_zero":       # the loose general formulas with a component that is k p, not 0
                    assert st.way == "loose" and st.filter[0] and B.value(st.pp[0]) % B.P == 0 and B.value(st.pp[0]) > 0
                    assert B.value(st.pp[1]) % B.P
                else:
                    assert st.way == "false_positive" and st.filter == (True, True)
                    assert (B.value(st.pp[1]) % B.P == 0) == (mode == "c0_alias_c1_equal") and B.value(st.pp[0]) % B.P
    f1, f2 = B.g1_family(rng, 12), B.g2_family(rng, 8)
    for fam in (f1, f2):
        assert len({q[0] for q in fam}) == len(fam)
        assert all(B.pair_ways(a, b) == ("false_positive", "false_positive") for i, a in enumerate(fam) for b in fam[i + 1:])
        got, _ = real_chain(hs, fam)
        assert got == oracle_sum(fam)
    s1, s2 = B.g1_saturated(8), B.g2_saturated(6)
    assert all(B.is_saturated(q) and O.bls_g1_on_curve(q) for q in s1) and all(B.is_saturated(q) and O.bls_g2_on_curve(q) for q in s2)
    for sat, rnd in ((s1, B.random_g1), (s2, B.random_g2)):
        pts = sat + [rnd(rng), sat[0], rnd(rng), sat[1]]
        got, _ = real_chain(hs, pts)
        assert got == oracle_sum(pts)


def test_false_positive_against_a_loose_accumulator(hs):
    """Chains of three and more points whose LAST point passes the filter against an accumulator that is no longer canonical
    (zz != 1, x unreduced), and chains that double or cancel there: the fallback must canonicalise before it uses the exact
    formulas. G1 and G2, against the oracle's sum, the LooseBound limits checked after every addition. CPU only: the order inside
    a bucket is arbitrary on the device."""
    rng = np.random.default_rng(7)
    for rnd, add, neg in ((B.random_g1, O.bls_g1_add, lambda q: (q[0], B.P - q[1])),
                          (B.random_g2, O.bls_g2_add, lambda q: (q[0], ((B.P - q[1][0]) % B.P, (B.P - q[1][1]) % B.P)))):
        ways = []
        for length in (2, 2, 3, 5, 9):
            prefix = [rnd(rng) for _ in range(length)]
            q = B.loose_false_positive(prefix, rng)
            assert q is not None
            acc, _ = B.chain(prefix)
            assert max(B.value(c) for c in B.components(acc[0])) >= B.P or length == 2      # the accumulator is loose in fact
            for tail in ([], [rnd(rng), rnd(rng)]):
                pts = prefix + [q] + tail
                got, steps = real_chain(hs, pts)
                assert steps[length].way == "false_positive" and got == oracle_sum(pts)
            ways.append(steps[length].way)
        assert ways == ["false_positive"] * 5
        # doubling and cancellation against an unreduced accumulator
        found = 0
        while found < 4:
            prefix = [rnd(rng) for _ in range(2 + found % 3)]
            acc, _ = B.chain(prefix)
            if max(B.value(c) for c in B.components(acc[0])) < B.P:
                continue                      # x happens to be reduced: identity in place of xyzz_canon would go unseen
            found += 1
            s = oracle_sum(prefix)
            got, steps = real_chain(hs, prefix + [s, prefix[0]])
            assert steps[len(prefix)].way == "doubling" and got == add(add(s, s), prefix[0])
            got, steps = real_chain(hs, prefix + [neg(s), prefix[0]])
            assert steps[len(prefix)].way == "cancellation" and steps[len(prefix) + 1].way == "first" and got == prefix[0]


# ---- 5. every builder of the GPU cases ------------------------------------------------------------------------------------------------
PLANTED = {}


def record(family, case):
    PLANTED[family] = PLANTED.get(family, 0) + case.planted
    assert B.fill_share(case) >= MIN_SHARE, (family, case.planted, case.wanted)


@pytest.mark.parametrize("pattern", T.R1CS_PATTERNS)
def test_r1cs_builders(hs, pattern):
    case = T.general_case(pattern)
    s, wit = case.inputs, case.witnesses
    record("r1cs general terms + create", case)
    assert wit["short"] and wit["long"] and len(wit["create"]) == 2 and wit["small"]
    assert_fr_witnesses(hs, wit["short"] + wit["long"] + wit["create"])
    for c, _ in wit["create"]:
        assert c in s["coeffs"] and fr_raw(hs, 3, c, 0) == B.fr_mont(c)
    for w, c in wit["small"]:
        assert B.mul_small(w, c).n_sub == 1 and small_raw(hs, w, c) == w * c % B.R
    PLANTED["r1cs mul_small pairs"] = PLANTED.get("r1cs mul_small pairs", 0) + len(wit["small"])
    # the witnesses are terms of the system: (coefficient in Montgomery form, wire value)
    terms = set()
    for m in (0, 2):
        _, col, cf = s["mats"][m]
        terms |= {(B.fr_mont(s["coeffs"][k]), s["w"][c]) for c, k in zip(col.tolist(), cf.tolist())}
    assert all(pair in terms for pair in wit["short"] + wit["long"])
    _, col, cf = s["mats"][1]
    small_terms = {(s["w"][c], min(s["coeffs"][k], B.R - s["coeffs"][k])) for c, k in zip(col.tolist(), cf.tolist())}
    assert all(pair in small_terms for pair in wit["small"])
    lens = [int(p[0][7 + 1] - p[0][7]) for p in s["mats"][:1]] + [int(s["mats"][1][0][301] - s["mats"][1][0][300])]
    assert min(lens) > B.LONG_ROW_THRESHOLD and len(wit["long"]) >= MIN_SHARE * int(B.patterns(lens[0])[pattern].sum())
    prod = T.product_case(pattern)
    record("r1cs check products", prod)
    ps, broken = prod.inputs
    assert_fr_witnesses(hs, prod.witnesses)
    w = ps["w"]
    assert all(w[3 * j + 1] * w[3 * j + 2] % B.R == w[3 * j + 3] for j in range(ps["n"])) and broken == sorted(set(broken)) and len(broken) >= 3
    assert {(w[3 * j + 1], w[3 * j + 2]) for j in range(ps["n"])} >= set(prod.witnesses)


@pytest.mark.parametrize("log_n,site,pattern", T.NTT_CASES)
def test_ntt_builders(hs, log_n, site, pattern):
    case = T.ntt_case(log_n, site, pattern)
    assert case is not None
    record("fr_ntt " + site, case)
    assert_fr_witnesses(hs, case.witnesses[:: max(1, len(case.witnesses) // 256)])
    assert all(B.fr_subtracts(a, b) for a, b in case.witnesses)
    inp = case.inputs
    x = B.fr_ints(inp["values"])
    assert all(v < B.R for v in x)
    n = 1 << log_n
    if site == "load":
        assert {a for a, _ in case.witnesses} <= set(x)
    elif site == "coset_scale":
        ops = {(B.fr_mont(v), B.fr_mont(up)) for v, up in zip(x, B.powers(B.COSET_SHIFT, n))}
        assert set(case.witnesses) <= ops
    elif site in ("first_stage", "second_kernel", "third_kernel"):
        plan = B.ntt_plan(log_n)
        s = inp["stages_before"]
        assert s == plan[B.NTT_SITES.index(site) - 2][1] and (s == 0) == (site == "first_stage")
        y, L = inp["intermediate"], n >> s
        h = L // 2
        w = B.root(log_n, inp["inverse"])
        tw = [B.fr_mont(t) for t in B.powers(pow(w, 1 << s, B.R), h)]
        pairs = {(B.fr_mont((y[lo] - y[lo + h]) % B.R), tw[lo % L]): lo for lo in range(n) if lo % L < h}
        assert set(case.witnesses) <= set(pairs)
        if log_n <= 11:       # the intermediate array is what the first s stages leave
            assert B.dif_stages(x, log_n, s, inp["inverse"]) == y
        else:                 # ... checked on the planted pairs (a sample) from the 2^s inputs each depends on
            for wit in case.witnesses[:: max(1, len(case.witnesses) // 24)]:
                lo = pairs[wit]
                assert B.after_stages_at(x, log_n, s, lo, inp["inverse"]) == y[lo] and B.after_stages_at(x, log_n, s, lo + h, inp["inverse"]) == y[lo + h]
    else:
        out = inp["output"]
        ops = {(B.fr_mont(v * up % B.R), B.fr_mont(down)) for v, up, down in zip(out, B.powers(B.COSET_SHIFT, n), B.powers(B.COSET_INV, n))}
        assert set(case.witnesses) <= ops
        assert (O.fr_ntt(inp["values"], inverse=True, shift=inp["shift"]) == B.fr_rows(out)).all()


def test_constants_that_admit_no_operand():
    """Montgomery one (the twiddle omega^0, the coset power shift^0) and the 1/n scale of the inverse transform's store are
    s = 2^(280 - k) mod r (k = log n; k = 0 is one). Write 2^(280 - k) = j r + s. For 0 < a < r, e = a s r^-1 mod 2^280 is
    t 2^(280 - k) - a j with t = a r^-1 mod 2^k and 0 < a j < 2^(280 - k); T >= r needs e <= a s / r < r, so t = 1 and
    a (j + s / r) >= 2^(280 - k) = r (j + s / r): a >= r. No operand subtracts against these constants: their products are
    never planted, and the final subtraction there is dead code for canonical inputs. The search agrees."""
    rng = np.random.default_rng(8)
    for k in (0, 1, 10, 11, 18, 28):
        s = B.fr_mont(pow(1 << k, -1, B.R))
        assert s == (1 << (280 - k)) % B.R and B.plant_fr(s, rng) is None
        assert not any(B.fr_subtracts(a, s) for a in B.fr_random(rng, 4000) + [B.R - 1 - i for i in range(200)])


def test_ntt_plan_names_the_kernels():
    assert [k for k, _ in B.ntt_plan(10)] == ["tile<true,true>"]
    assert B.ntt_plan(11) == [("colpass<true>", 0), ("tile<false,true>", 1)]
    assert B.ntt_plan(17) == [("colpass<true>", 0), ("tile<false,true>", 7)]
    assert B.ntt_plan(18) == [("colpass<true>", 0), ("colpass<false>", 4), ("tile<false,true>", 8)]


@pytest.mark.parametrize("log_n,pattern", T.QUOTIENT_CASES)
def test_quotient_builders(hs, log_n, pattern):
    case = T.quotient_case(log_n, pattern)
    record("groth16 quotient", case)
    assert_fr_witnesses(hs, case.witnesses)
    inp = case.inputs
    ca, cb, cc = inp["coset"]
    for k, ev in zip("abc", (ca, cb, cc)):      # the coset evaluations of the inputs are the chosen ones
        coeffs = O.fr_ntt(inp[k], inverse=True)
        assert (O.fr_ntt(coeffs, shift=B.COSET_SHIFT) == B.fr_rows(ev)).all()
    den = B.fr_mont(pow(pow(B.COSET_SHIFT, 1 << log_n, B.R) - 1, -1, B.R))
    ops = {(B.fr_mont(a), B.fr_mont(b)) for a, b in zip(ca, cb)} | {(B.fr_mont((a * b - c) % B.R), den) for a, b, c in zip(ca, cb, cc)}
    assert set(case.witnesses) <= ops and len(case.witnesses) == 2 * case.planted


@pytest.mark.parametrize("group,layout,mode", T.MSM_PAIR_CASES)
def test_msm_pair_builders(group, layout, mode):
    case = T.pairs_case(group, layout, mode)
    record("msm G%d two-point buckets" % group, case)
    ks, pts = case.inputs
    on = O.bls_g1_on_curve if group == 1 else O.bls_g2_on_curve
    assert all(on(q) for q in pts) and len(pts) <= 1023 and max(ks) < 1 << 255
    want = ("loose", "loose") if mode == "c0_zero" else ("false_positive", "false_positive")
    buckets = {}
    for k, q in zip(ks, pts):
        buckets.setdefault(k, []).append(q)
    assert all(len(b) == 2 for b in buckets.values()) and len(buckets) == {"one": 1, "wave": 64, "alternate": 128}[layout]
    in_buckets = {frozenset(b) for b in buckets.values()}
    for a, b in case.witnesses:
        assert B.pair_ways(a, b) == want and frozenset((a, b)) in in_buckets
        if mode == "c0_zero":
            st = B.chain([a, b])[1][1]
            assert st.filter[0] and B.value(st.pp[0]) % B.P == 0
    # a bucket scalar is one digit of one window: no carry into the next
    assert all(k == (k >> (5 * w) & 31) << (5 * w) and 1 <= (k >> (5 * w) & 31) <= 16 for k in buckets for w in [(k.bit_length() - 1) // 5])


@pytest.mark.parametrize("group", [1, 2])
def test_msm_heavy_and_saturated_builders(group):
    on = O.bls_g1_on_curve if group == 1 else O.bls_g2_on_curve
    case = T.heavy_case(group)
    record("msm G%d heavy bucket" % group, case)
    ks, pts = case.inputs
    fam = case.witnesses
    assert len(fam) > (256 if group == 1 else 128) and len(fam) > B.msm_heavy_limit(len(pts)) and len({q[0] for q in fam}) == len(fam)
    assert all(on(q) for q in pts[:: 7])
    rng = np.random.default_rng(group)
    for _ in range(40):       # pairwise: any two, either order (every x is base + d p in the low limb, d in 0..7)
        i, j = rng.choice(len(fam), 2, replace=False)
        assert B.pair_ways(fam[i], fam[j]) == ("false_positive", "false_positive")
    mx = [B.mont_x(q) for q in fam]
    base = mx[0] if group == 1 else mx[0][0]
    assert all(((x if group == 1 else x[0]) - base) * B.PINV28 % (1 << 28) in set(range(8)) | set(range((1 << 28) - 7, 1 << 28)) for x in mx)
    case = T.saturated_case(group)
    record("msm G%d saturated limbs" % group, case)
    ks, pts = case.inputs
    assert all(B.is_saturated(q) and on(q) for q in case.witnesses) and set(case.witnesses) <= set(pts)
    assert ks.count(3) > B.msm_heavy_limit(len(pts)) and len(pts) <= 1023
    assert sum(1 for q in pts if not B.is_saturated(q)) == 16


def test_zz_planted_counts_are_reported():
    """(runs last in this file) what reached the device, per kernel family"""
    for k in sorted(PLANTED):
        print("%-34s %7d planted" % (k, PLANTED[k]))
    assert not PLANTED or min(PLANTED.values()) > 0
