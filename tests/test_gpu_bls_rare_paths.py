"""The rare paths of the BLS12-381 arithmetic, driven inside every kernel family of the Groth16 side through the public ABI: the
final subtraction of fr_mul (taken about once in 2^27 uniform products) in the R1CS evaluation and check, the F_r transforms and
the quotient; the one subtraction of mul_small; the 28-bit "same x?" filter of the loose bucket accumulation passing on different
points (2^-23 per F_p component) in ordinary and heavy buckets of both groups; saturated-limb coordinates; heavy buckets of
several chunks. Inputs and their host-side witnesses: tests/bls_rare_paths.py (checked on the CPU by tests/test_bls_rare_paths.py,
which builds every case of the lists below). Every comparison is equality of 64-bit words against the oracle or Python integers."""
import functools

import numpy as np
import pytest

import bls_rare_paths as B
import oracle_lib as O
import r1cs_cases as RC

pytestmark = pytest.mark.gpu

R1CS_PATTERNS = B.PATTERNS
# (log_n, site, pattern): log_n 10 is k_tile<true,true> alone, 11 adds k_colpass<true>, 18 is the smallest size with
# k_colpass<false> (one sparse pattern there: a planted element costs a lattice reduction)
NTT_CASES = ([(10, site, pat) for site in ("load", "coset_scale", "first_stage", "store_coset") for pat in B.PATTERNS if (site, pat) != ("first_stage", "lane0")]
             + [(11, site, pat) for site in ("load", "first_stage", "second_kernel") for pat in B.PATTERNS if (site, pat) != ("second_kernel", "lane0")]
             + [(11, site, "alternate") for site in ("coset_scale", "store_coset")]
             + [(18, site, "lane63") for site in ("load", "first_stage", "second_kernel", "third_kernel", "store_coset")])
# The store's 1/n scale is not in the list: no operand subtracts against it (tests/test_bls_rare_paths.py proves it).
# (no lane0 pattern where an eighth of those lanes hold the twiddle omega^0, which admits no operand: the butterflies of 512 pairs)
QUOTIENT_CASES = [(10, pat) for pat in B.PATTERNS]
MSM_PAIR_CASES = ([(1, layout, "both") for layout in ("one", "wave", "alternate")]
                  + [(2, layout, "both") for layout in ("one", "wave", "alternate")]
                  + [(2, "wave", "c0_zero"), (2, "wave", "c0_alias_c1_equal"), (2, "alternate", "c0_zero"), (2, "alternate", "c0_alias_c1_equal")])


def seed_of(*key):
    return sum((i + 1) * sum(str(k).encode()) for i, k in enumerate(key)) % (1 << 31)


@functools.lru_cache(maxsize=None)
def ntt_case(log_n, site, pattern):
    return B.ntt_case(log_n, site, pattern, seed_of(log_n, site, pattern), O.fr_ntt)


@functools.lru_cache(maxsize=None)
def quotient_case(log_n, pattern):
    return B.quotient_case(log_n, pattern, seed_of(log_n, pattern), O.fr_ntt)


@functools.lru_cache(maxsize=None)
def general_case(pattern):
    return B.r1cs_general_case(pattern, seed_of("general", pattern))


@functools.lru_cache(maxsize=None)
def product_case(pattern):
    return B.r1cs_product_case(pattern, seed_of("product", pattern))


@functools.lru_cache(maxsize=None)
def pairs_case(group, layout, mode):
    return B.msm_pairs_case(group, layout, seed_of(group, layout, mode), mode)


@functools.lru_cache(maxsize=None)
def heavy_case(group):
    return B.msm_heavy_case(group, seed_of("heavy", group))


@functools.lru_cache(maxsize=None)
def saturated_case(group):
    _, r, G = O.bls_constants()
    rng = np.random.default_rng(77 + group)
    ks = [int.from_bytes(rng.bytes(32), "little") % r for _ in range(16)]
    gens = [O.bls_g1_mul(G, k) for k in ks] if group == 1 else [O.bls_g2_mul(O.bls_g2_generator(), k) for k in ks]
    return B.msm_saturated_case(group, seed_of("saturated", group), gens)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


# ---- R1CS ----------------------------------------------------------------------------------------------------------------------------
def make(prover, s):
    import cityprover as cp
    return cp.R1cs(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"])


@pytest.mark.parametrize("pattern", R1CS_PATTERNS)
def test_r1cs_planted_terms_evaluate_and_check_as_python_does(prover, pattern):
    """k_eval_short and k_eval_long with general terms whose product subtracts and one-limb terms that need mul_small's
    subtraction, coefficients whose conversion at create subtracts; then the fused check (row_value) on the same rows"""
    case = general_case(pattern)
    s = case.inputs
    r1cs = make(prover, s)
    assert r1cs.info.n_long_rows == 2 and min(r1cs.info.n_terms_class[3:6]) > 0      # small, negative-small and general terms
    dw = prover.to_device(RC.limbs4(s["w"]))
    got = r1cs.eval(dw.ptr)
    want = RC.eval_all(s)
    for m in range(3):
        assert (got[m] == RC.limbs4(want[m] + [0] * (r1cs.n_pad - s["n"]))).all(), "matrix %d" % m
    bad = [j for j in range(s["n"]) if want[0][j] * want[1][j] % B.R != want[2][j]]
    assert r1cs.check(dw.ptr) == (len(bad), bad[0])
    dw.free(); r1cs.free()


@pytest.mark.parametrize("pattern", R1CS_PATTERNS)
def test_check_multiplies_planted_rows_exactly(prover, pattern):
    """rows w_x * w_y = w_z whose product subtracts inside k_check, which compares limb by limb: satisfied means zero
    violations, w_z + 1 is counted with the right lowest row; by the fused route and by the evaluate-then-check route of
    cp_groth16_prove_r1cs_bls12381 (which refuses a violated witness before it reads the key)"""
    import cityprover as cp
    s, broken = product_case(pattern).inputs
    r1cs = make(prover, s)
    dw = prover.to_device(RC.limbs4(s["w"]))
    assert r1cs.check(dw.ptr) == (0, None)
    w = list(s["w"])
    for j in broken:
        w[3 * j + 3] = (w[3 * j + 3] + 1) % B.R
    db = prover.to_device(RC.limbs4(w))
    assert r1cs.check(db.ptr) == (len(broken), broken[0])
    pk = cp.Groth16Pk()
    pk.n_wires, pk.n_private, pk.log_domain = s["n_wires"], s["n_wires"] - 1, r1cs.info.log_domain
    with pytest.raises(cp.CityProverError, match=r"%d of %d constraints violated, the first is constraint %d\b" % (len(broken), s["n"], broken[0])):
        cp.groth16_prove_r1cs(prover, pk, r1cs, db.ptr, 1, 1)
    dw.free(); db.free(); r1cs.free()


# ---- F_r NTT and the Groth16 quotient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,site,pattern", NTT_CASES)
def test_fr_ntt_with_planted_products(prover, log_n, site, pattern):
    import cityprover as cp
    case = ntt_case(log_n, site, pattern)
    inp = case.inputs
    got = cp.fr_ntt(prover, inp["values"], inverse=inp["inverse"], shift=inp["shift"])
    assert (got == O.fr_ntt(inp["values"], inverse=inp["inverse"], shift=inp["shift"])).all()
    if "output" in inp:
        assert B.fr_ints(got) == inp["output"]


@pytest.mark.parametrize("log_n,pattern", QUOTIENT_CASES)
def test_groth16_quotient_with_planted_products(prover, log_n, pattern):
    import cityprover as cp
    inp = quotient_case(log_n, pattern).inputs
    assert (cp.groth16_quotient(prover, inp["a"], inp["b"], inp["c"]) == O.groth16_quotient(inp["a"], inp["b"], inp["c"])).all()


# ---- MSM -------------------------------------------------------------------------------------------------------------------------------
def msm_both(prover, group, ks, pts):
    import cityprover as cp
    sc = B.scalar_rows(ks)
    O.lib().or_set_threads(8)
    try:
        if group == 1:
            return cp.msm_g1(prover, sc, B.g1_rows(pts)), O.bls_g1_msm(sc, B.g1_rows(pts))
        return cp.msm_g2(prover, sc, B.g2_rows(pts)), O.bls_g2_msm(sc, B.g2_rows(pts))
    finally:
        O.lib().or_set_threads(1)


@pytest.mark.parametrize("group,layout,mode", MSM_PAIR_CASES)
def test_msm_two_point_buckets_of_filter_false_positives(prover, group, layout, mode):
    ks, pts = pairs_case(group, layout, mode).inputs
    assert len(pts) <= 1023
    got, want = msm_both(prover, group, ks, pts)
    assert got == want and want is not None


@pytest.mark.parametrize("group", [1, 2])
def test_msm_heavy_bucket_of_pairwise_false_positives(prover, group):
    ks, pts = heavy_case(group).inputs
    assert ks.count(1) > B.msm_heavy_limit(len(pts)) and len(pts) <= 1023
    got, want = msm_both(prover, group, ks, pts)
    assert got == want and want is not None


@pytest.mark.parametrize("group", [1, 2])
def test_msm_saturated_limb_points(prover, group):
    ks, pts = saturated_case(group).inputs
    assert ks.count(3) > B.msm_heavy_limit(len(pts)) and len(pts) <= 1023
    got, want = msm_both(prover, group, ks, pts)
    assert got == want and want is not None


@pytest.mark.parametrize("group", [1, 2])
def test_msm_heavy_bucket_of_three_chunks(prover, group):
    """20 000 distinct points with one scalar: a single bucket of more than 2 x 8192 points, so k_heavy_combine adds three chunk
    sums. Closed form: k * sum (3 i + 5) G."""
    import cityprover as cp
    _, r, G = O.bls_constants()
    n, k = 20_000, 1
    assert n > 2 * B.HEAVY_CHUNK and n > B.msm_heavy_limit(n, 13)
    gen = G if group == 1 else O.bls_g2_generator()
    P = (cp.G1Points if group == 1 else cp.G2Points).synthetic(prover, gen, 3, 5, n)
    ds = prover.to_device(B.scalar_rows([k] * n))
    got = P.msm_dev(ds.ptr)
    ds.free(); P.free()
    total = k * sum(3 * i + 5 for i in range(n)) % r
    assert got == (O.bls_g1_mul(G, total) if group == 1 else O.bls_g2_mul(gen, total))
