"""CPU tests of the DEFINITION of an AIR constraint (tests/air_semantics.py: Python integers, row by row) and of the inputs the GPU
tests of the same name prove: the interpreter against the oracle's row interpreter on random programs; the hand-written table
"kind k binds row r" against the interpreter over the whole corruption list of the probe AIR; the oracle's prover and verifier
against that verdict, quotient_degree_bits = 0 included; the degree bound of the quotient. No tolerance anywhere: equality of
64-bit words or of an accept / refuse verdict."""
import numpy as np
import pytest

import air_programs as A
import air_semantics as S
import oracle_lib as O

P = O.P
SHAPES = [(3, 0, 1), (4, 0, 1), (4, 1, 1), (5, 0, 2), (5, 2, 2)]   # (degree_bits, quotient_degree_bits, rate_bits)


def fri_of(db, rb):
    return (db, rb, 1, 3, 5, (1,))


def probe_case(db, top, seed=None):
    trace, pub, glo = S.honest_trace(db, 700 + db if seed is None else seed)
    cases = S.corruptions(trace, pub)
    assert len(cases) == S.N_CORRUPTIONS == 37
    return trace, pub, glo, cases


# ---- (a) the interpreter against the oracle's ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_interpreter_equals_the_oracle_row_interpreter(seed):
    rng = np.random.default_rng(3100 + seed)
    k = int(rng.integers(3, 12))
    b = A.random_program(3200 + seed, k, int(rng.integers(40, 300)), max_degree=3)
    op = b.oracle()
    assert op.check() == 0
    n = 16
    trace = rng.integers(0, P, (k, n), dtype=np.uint64)
    trace[:, [2, 3, n - 1]] = 0                     # rows that are zero, their successors and the wrap: sinks without a uniform term vanish there
    pub, glo, cha = ([int(v) for v in rng.integers(0, P, c, dtype=np.uint64)] for c in (b.n_public, b.n_global, b.n_challenge))
    values, kinds, degrees = S.sink_values(b, trace, pub, glo, cha)
    want_kinds = [S.KIND_OF[o] for (o, _, _, _) in b.ops if o in S.KIND_OF]
    assert kinds == want_kinds and len(kinds) == op.num_constraints()
    zeros = 0
    for r in range(n):
        vals = op.eval_row(trace[:, r], trace[:, (r + 1) % n], pub, glo, cha)
        got = [int(vals[a]) for (o, a, _, _) in b.ops if o in S.KIND_OF]
        assert got == [values[s][r] for s in range(len(kinds))], r
        # over F_p^2 on (v, 0) pairs as well: what a verifier's interpreter computes
        pair = lambda v: np.stack([np.asarray(v, dtype=np.uint64), np.zeros(len(v), np.uint64)], axis=1)
        ext, ek = op.eval_ext(pair(trace[:, r]), pair(trace[:, (r + 1) % n]), pair(pub), pair(glo), pair(cha))
        assert [int(x) for x in ext[:, 0]] == got and not ext[:, 1].any()
        assert [S.KIND_OF[int(x)] for x in ek] == kinds
        zeros += sum(v == 0 for v in got)
    viol, deg2 = S.violations(b, trace, pub, glo, cha)
    assert deg2 == degrees
    assert viol == sorted((s, kinds[s], r) for s in range(len(kinds)) for r in range(n) if values[s][r] and S.binds(kinds[s], r, n))
    assert 0 < zeros and len(viol) > 0              # both verdicts occur


# ---- (b) the hand-written table against the interpreter ------------------------------------------------------------------
@pytest.mark.parametrize("top", [False, True])
@pytest.mark.parametrize("db,q,rb", SHAPES)
def test_hand_table_equals_the_interpreter(db, q, rb, top):
    n = 1 << db
    b = S.probe_air(q, db, top)
    trace, pub, glo, cases = probe_case(db, top)
    viol, degrees = S.violations(b, trace, pub, glo)
    assert viol == []
    kinds = [k for _, k, _ in S.PROBE_SINKS]
    hi, lo = ((1 << q) + 1, 1 << q) if top else (1, 1)
    assert degrees == [hi, hi, lo, lo, 1, 1, 1, 1, 1]
    # the honest trace does break every sink where its kind does not bind: the selectors are what makes it honest
    values, got_kinds, _ = S.sink_values(b, trace, pub, glo)
    assert got_kinds == kinds
    assert values[1][n - 1] and all(values[2][1:]) and all(values[3][:n - 1]) and values[4][n - 1] and values[6][1] and values[8][0]
    accepted = 0
    for name, c, r, t, pb in cases:
        got, _ = S.violations(b, t, pb, glo)
        assert got == S.expected_violations(c, r, n, name), name
        accepted += not got
    assert accepted == 1 + 4 + 4                    # c1 at n - 1, c2 off row 0, c3 off row n - 1


# ---- (c) the oracle's prover and verifier -----------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [False, True])
@pytest.mark.parametrize("db,q,rb", SHAPES)
def test_oracle_verifier_accepts_iff_no_violation(db, q, rb, top):
    b = S.probe_air(q, db, top)
    trace, pub, glo, cases = probe_case(db, top)
    od, keep = O.stark_desc(db, q, 2, O.fri_params(*fri_of(db, rb)), S.N_COLUMNS, b.oracle(), n_public=S.N_PUBLIC, n_global=S.N_GLOBAL)
    verdicts = []
    for name, c, r, t, pb in [("honest", None, None, trace, pub)] + cases:
        proof = O.stark_prove(od, t, O.challenger_new(), publics=pb, globals_=glo)
        rc = O.stark_verify(od, O.challenger_new(), proof, publics=pb, globals_=glo)
        viol, _ = S.violations(b, t, pb, glo)
        assert rc == (2 if viol else 0), (name, rc, viol)     # every refusal is the identity at zeta
        verdicts.append(rc)
    assert verdicts.count(0) == 10 and len(verdicts) == 38


# ---- (d) the degree bound of the quotient ----------------------------------------------------------------------------------
def quotient_coeffs(b, trace, q, rb, pub, glo, alphas):
    ob = O.Batch(trace, rb, 1)
    try:
        out = O.air_quotient(b.oracle(), [ob], q, alphas, pub, glo)
    finally:
        ob.close()
    return out.reshape(len(alphas), -1)             # the 2^q chunks of n of one alpha are consecutive


@pytest.mark.parametrize("top", [False, True])
@pytest.mark.parametrize("db,q,rb", SHAPES)
def test_quotient_degree_bound(db, q, rb, top):
    n, M = 1 << db, 1 << (db + q)
    b = S.probe_air(q, db, top)
    trace, pub, glo, cases = probe_case(db, top)
    _, degrees = S.violations(b, trace, pub, glo)
    bound = S.quotient_degree_bound(degrees, [k for _, k, _ in S.PROBE_SINKS], n)
    # without the mask the first / last row sinks decide: 2 (n - 1) - n; with it the transition sink: (2^q + 1)(n - 1) + 1 - n
    assert bound == (M - (1 << q) if top else n - 2)
    alphas = [int(v) for v in np.random.default_rng(5).integers(1, P, 3, dtype=np.uint64)]
    honest = quotient_coeffs(b, trace, q, rb, pub, glo, alphas)
    assert honest.shape == (3, M)
    assert not honest[:, bound + 1:].any()
    assert all(honest[a, bound] for a in range(3))  # the bound is reached: it is the highest coefficient that MAY be non-zero
    if bound < M - 1:                               # at q = 0 the masked sinks fill all n coefficients: nothing lies above
        bad = quotient_coeffs(b, cases[2][3], q, rb, pub, glo, alphas)   # c0 at row n / 2
        assert cases[2][0] == "c0@%d" % (n // 2)
        assert all(bad[a, bound + 1:].any() for a in range(3))
    else:
        assert (q, top) == (0, True)


# ---- (e) random programs at q = 0 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_oracle_quotient_of_random_degree_2_programs_at_q_0(seed):
    rng = np.random.default_rng(3300 + seed)
    db, rb, k = int(rng.integers(2, 7)), int(rng.integers(1, 4)), int(rng.integers(2, 10))
    b = A.random_program(3400 + seed, k, int(rng.integers(30, 200)), max_degree=2)
    trace = rng.integers(0, P, (k, 1 << db), dtype=np.uint64)
    pub, glo, cha = (rng.integers(0, P, c, dtype=np.uint64) for c in (b.n_public, b.n_global, b.n_challenge))
    ob = O.Batch(trace, rb, 0)
    try:
        out = O.air_quotient(b.oracle(), [ob], 0, rng.integers(0, P, 2, dtype=np.uint64), pub, glo, cha)
    finally:
        ob.close()
    assert out.shape == (2, 1 << db) and out.any() and (out < P).all()
