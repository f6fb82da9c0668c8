"""The device-resident R1CS (cp_r1cs_bls12381_*, cp_groth16_prove_r1cs_bls12381) against Python integers modulo r: every
evaluation of A w, B w, C w compared word for word, the launch classes proven from the profile, the satisfaction check against
a recount in Python, the proof from a witness alone against the trapdoor and against cp_groth16_prove_bls12381 fed
Python-computed evaluations. Systems: tests/r1cs_cases.py. No tolerance anywhere: every comparison is equality of 64-bit words."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
R = RC.R


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def make(prover, s, flags=0):
    import cityprover as cp
    return cp.R1cs(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], flags)


def evaluate(prover, r1cs, dw):
    """eval_dev into buffers that held garbage before: the zero padding has to be written, not found"""
    n_pad = r1cs.n_pad
    junk = np.full((n_pad, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    bufs = [prover.to_device(junk) for _ in range(3)]
    r1cs.eval_dev(dw.ptr, *(b.ptr for b in bufs))
    out = [b.download().reshape(n_pad, 4) for b in bufs]
    for b in bufs:
        b.free()
    return out


def expect(s, n_pad):
    want = RC.eval_all(s)
    return [RC.limbs4(v + [0] * (n_pad - s["n"])) for v in want]


# ---- 1. evaluation parity, every row ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 64, 1000, 4097, 1 << 16])
def test_every_row_of_every_matrix_equals_python(prover, n):
    s = RC.random_system(n, seed=1000 + n)
    lens = np.concatenate([RC.row_lengths(s, m) for m in range(3)])
    assert lens.max() == 100_000 and (lens == 5_000).any() and (lens == 0).any()       # what every size holds (r1cs_cases.random_system)
    if n >= 3:
        assert (lens == 1).any() and (lens == RC.LONG_ROW_THRESHOLD).any() and (lens == RC.LONG_ROW_THRESHOLD + 1).any()
    r1cs = make(prover, s)
    info = r1cs.info
    assert (info.n_constraints, info.n_wires, info.n_coeffs) == (n, s["n_wires"], len(s["coeffs"]))
    assert info.log_domain == max(0, (n - 1).bit_length()) and r1cs.n_pad >= n
    assert list(info.nnz) == [len(m[1]) for m in s["mats"]]
    assert info.longest_row == max(int(RC.kept_lengths(s, m).max()) for m in range(3)) > 90_000     # terms kept: zero coefficients are dropped
    assert info.long_row_threshold == RC.LONG_ROW_THRESHOLD
    assert info.n_long_rows == len(RC.long_rows(s)) and info.n_short_rows == 3 * n - info.n_long_rows
    assert sum(info.n_terms_class) == sum(info.nnz) and info.n_terms_class[0] > 0
    w = RC.limbs4(s["w"])
    dw = prover.to_device(w)
    got = evaluate(prover, r1cs, dw)
    want = expect(s, r1cs.n_pad)
    for m in range(3):
        bad = np.nonzero((got[m] != want[m]).any(axis=1))[0]
        assert bad.size == 0, ("matrix %d" % m, bad[:8], RC.row_lengths(s, m)[bad[:8][bad[:8] < n]])
    assert (dw.download().reshape(-1, 4) == w).all(), "the witness was written"
    again = evaluate(prover, r1cs, dw)
    assert all((x == y).all() for x, y in zip(got, again))
    # the same system with every term on the general path (the A/B switch of the measurement) computes the same
    plain = make(prover, s, flags=1)
    assert plain.info.n_terms_class[5] == sum(plain.info.nnz)
    got_plain = evaluate(prover, plain, dw)
    assert all((x == y).all() for x, y in zip(got, got_plain))
    plain.free(); r1cs.free(); dw.free()


# ---- 2. the launch classes --------------------------------------------------------------------------------------------------------
def test_short_and_long_rows_take_their_own_kernels(prover):
    for with_long, labels in ((True, {"r1cs_eval_short", "r1cs_eval_long"}), (False, {"r1cs_eval_short"})):
        s = RC.random_system(300, seed=7, with_long=with_long)
        assert bool(RC.long_rows(s)) == with_long
        r1cs = make(prover, s)
        dw = prover.to_device(RC.limbs4(s["w"]))
        bufs = [prover.alloc(4 * r1cs.n_pad) for _ in range(3)]
        prover.profile_begin()
        r1cs.eval_dev(dw.ptr, *(b.ptr for b in bufs))
        prof = prover.profile_end()
        assert {k for k in prof if k.startswith("r1cs_")} == labels
        assert all(prof[k]["launches"] == 1 for k in labels)      # one launch per class, the three matrices together
        prover.profile_begin()
        r1cs.check(dw.ptr)
        prof = prover.profile_end()
        assert {k for k in prof if k.startswith("r1cs_")} == ({"r1cs_check", "r1cs_eval_long"} if with_long else {"r1cs_check"})
        for b in bufs + [dw]:
            b.free()
        r1cs.free()


# ---- 3. at the size it is timed ----------------------------------------------------------------------------------------------------
def test_two_to_the_twenty_constraints(prover):
    """2^20 constraints: every long row and a seeded sample of 4 096 other rows against Python; the rest by check_dev = 0
    violations on the satisfied witness (a row that evaluated wrongly breaks a b = c)."""
    n = 1 << 20
    s = RC.satisfied_system(n, seed=20)
    r1cs = make(prover, s)
    dw = prover.to_device(RC.limbs4(s["w"]))
    got = evaluate(prover, r1cs, dw)
    longs = RC.long_rows(s)
    assert len(longs) == 4 and r1cs.info.n_long_rows == 4 and r1cs.info.longest_row == max(int(RC.kept_lengths(s, m).max()) for m in range(3)) > 90_000
    rng = np.random.default_rng(2020)
    rows = [(m, int(j)) for m in range(3) for j in rng.choice(n, 4096 // 3 + 1, replace=False)][:4096] + longs
    for m, j in rows:
        assert RC.from_limbs4(got[m][j])[0] == RC.eval_row(s, m, j), (m, j)
    assert r1cs.check(dw.ptr) == (0, None)
    r1cs.free(); dw.free()


# ---- 4. the check -------------------------------------------------------------------------------------------------------------------
def test_check_counts_what_python_counts(prover):
    n = 3000                                     # not a power of two: 1 096 padding rows that must never count
    s = RC.satisfied_system(n, seed=4, long_lengths=(5_000, 100_000, 300))
    assert RC.violated_rows(s) == []
    r1cs = make(prover, s)
    assert r1cs.n_pad == 4096

    def check_with(w):
        dw = prover.to_device(RC.limbs4(w))
        got = r1cs.check(dw.ptr)
        dw.free()
        return got

    assert check_with(s["w"]) == (0, None)
    cases = {}
    # one private input wire changed
    cases["input"] = 9
    # the last wire: only the C row of the last real constraint names it
    cases["last"] = s["n_wires"] - 1
    # a wire of the 100 000-term row
    m, j = 1, n // 3
    assert RC.row_lengths(s, m)[j] == 100_000
    lo = int(s["mats"][m][0][j])
    cases["long"] = int(next(c for c in s["mats"][m][1][lo:lo + 100_000] if c))
    for name, wire in cases.items():
        t = dict(s, w=list(s["w"]))
        t["w"][wire] = (t["w"][wire] + 1) % R
        bad = RC.violated_rows(t)
        assert bad, name
        if name == "last":
            assert bad == [n - 1]
        if name == "long":
            assert j in bad
        assert check_with(t["w"]) == (len(bad), bad[0]), name
    # the constant wire set to 2: most constraints break, many in every wave
    t = dict(s, w=[2] + list(s["w"][1:]))
    bad = RC.violated_rows(t)
    assert len(bad) > n // 4
    assert check_with(t["w"]) == (len(bad), bad[0])
    r1cs.free()


# ---- 5. proving from a witness alone ------------------------------------------------------------------------------------------------
def limbs(v, n):
    return [(int(v) >> (64 * i)) & (2**64 - 1) for i in range(n)]


def g1_rows(points):
    return np.array([limbs(P[0], 6) + limbs(P[1], 6) for P in points], dtype=np.uint64)


def g2_rows(points):
    return np.array([limbs(P[0][0], 6) + limbs(P[0][1], 6) + limbs(P[1][0], 6) + limbs(P[1][1], 6) for P in points], dtype=np.uint64)


@pytest.mark.parametrize("log_n,n_pub,n_in", [(3, 2, 3), (5, 3, 6)])
def test_proof_from_a_witness_matches_the_trapdoor_and_the_evaluations_route(prover, log_n, n_pub, n_in):
    import cityprover as cp
    _, r, G1 = O.bls_constants()
    G2 = O.bls_g2_generator()
    case = RC.groth16_case(log_n, n_pub, n_in)
    s = case["system"]
    w, m = s["w"], s["n_wires"]

    def pts1(logs):
        return [O.bls_g1_mul(G1, x) if x else G1 for x in logs], np.array([0 if x else 1 for x in logs], np.uint8)
    pa, a_inf = pts1(case["u"])
    pb1, b_inf = pts1(case["v"])
    pb2 = [O.bls_g2_mul(G2, x) if x else G2 for x in case["v"]]
    pk_, _ = pts1(case["k_log"])
    pz, _ = pts1(case["z_log"])
    sets = [cp.G1Points(prover, g1_rows(pa)), cp.G1Points(prover, g1_rows(pb1)), cp.G2Points(prover, g2_rows(pb2)),
            cp.G1Points(prover, g1_rows(pk_)), cp.G1Points(prover, g1_rows(pz))]
    flags = lambda f: prover.to_device(np.frombuffer(np.concatenate([f, np.zeros(-len(f) % 8, np.uint8)]).tobytes(), np.uint64))
    d_ainf, d_binf = flags(a_inf), flags(b_inf)
    pk = cp.Groth16Pk()
    pk.n_wires, pk.n_private, pk.log_domain = m, m - n_pub, log_n
    pk.a_g1, pk.b_g1, pk.b_g2, pk.k_g1, pk.z_g1 = (x.buf.ptr for x in sets)
    pk.a_inf, pk.b_inf = d_ainf.ptr, d_binf.ptr
    for name, P in (("alpha_g1", O.bls_g1_mul(G1, case["alpha"])), ("beta_g1", O.bls_g1_mul(G1, case["beta"])), ("delta_g1", O.bls_g1_mul(G1, case["delta"]))):
        getattr(pk, name)[:] = limbs(P[0], 6) + limbs(P[1], 6)
    for name, P in (("beta_g2", O.bls_g2_mul(G2, case["beta"])), ("delta_g2", O.bls_g2_mul(G2, case["delta"]))):
        getattr(pk, name)[:] = limbs(P[0][0], 6) + limbs(P[0][1], 6) + limbs(P[1][0], 6) + limbs(P[1][1], 6)
    r1cs = make(prover, s)
    assert r1cs.info.log_domain == log_n
    dw = prover.to_device(RC.limbs4(w))
    rr, ss = case["r"], case["s"]
    SENT = 0x5E5E5E5E5E5E5E5E
    out = [np.full(k, SENT, np.uint64) for k in (12, 24, 12)]
    A_pt, B_pt, C_pt = cp.groth16_prove_r1cs(prover, pk, r1cs, dw.ptr, rr, ss, out=out)
    assert A_pt == O.bls_g1_mul(G1, case["a_log"])
    assert B_pt == O.bls_g2_mul(G2, case["b_log"])
    assert C_pt == O.bls_g1_mul(G1, case["c_log"])
    assert (dw.download().reshape(-1, 4) == RC.limbs4(w)).all()
    # the same three points, word for word, from the evaluations Python computes
    ev = [prover.to_device(RC.limbs4(v)) for v in case["evals"]]
    ref = cp.groth16_prove(prover, pk, dw.ptr, ev[0].ptr, ev[1].ptr, ev[2].ptr, rr, ss)
    assert ref == (A_pt, B_pt, C_pt)
    flat = lambda P: [P[0][0], P[0][1], P[1][0], P[1][1]] if isinstance(P[0], tuple) else [P[0], P[1]]
    for words, P in zip(out, ref):
        assert words.tolist() == [x for c in flat(P) for x in limbs(c, 6)]
    # one witness value changed: refused, the first violated constraint named, the outputs left alone
    t = dict(s, w=list(w))
    t["w"][n_pub] = (t["w"][n_pub] + 1) % r
    bad = RC.violated_rows(t)
    assert bad
    dbad = prover.to_device(RC.limbs4(t["w"]))
    out = [np.full(k, SENT, np.uint64) for k in (12, 24, 12)]
    with pytest.raises(cp.CityProverError, match=r"does not satisfy the R1CS: %d of %d constraints violated, the first is constraint %d\b" % (len(bad), s["n"], bad[0])):
        cp.groth16_prove_r1cs(prover, pk, r1cs, dbad.ptr, rr, ss, out=out)
    assert all((o == SENT).all() for o in out)
    # a key that disagrees with the system
    pk.log_domain = log_n + 1
    with pytest.raises(cp.CityProverError, match="log_domain"):
        cp.groth16_prove_r1cs(prover, pk, r1cs, dw.ptr, rr, ss, out=out)
    pk.log_domain = log_n
    pk.n_wires = m + 1
    with pytest.raises(cp.CityProverError, match="n_wires"):
        cp.groth16_prove_r1cs(prover, pk, r1cs, dw.ptr, rr, ss, out=out)
    assert all((o == SENT).all() for o in out)
    for d in [dw, dbad, d_ainf, d_binf] + ev:
        d.free()
    for x in sets:
        x.free()
    r1cs.free()


# ---- 6. refusals of create -----------------------------------------------------------------------------------------------------------
def test_create_refuses_what_it_must(prover):
    import cityprover as cp
    base = RC.random_system(8, seed=6, with_long=False)
    coeffs = RC.limbs4(base["coeffs"])

    def refused(match, n=None, n_wires=None, coeffs_=None, mats=None, patch=None):
        mats_ = [tuple(a.copy() for a in m) for m in (mats or base["mats"])]
        if patch:
            patch(mats_)
        with pytest.raises(cp.CityProverError, match=match):
            cp.R1cs(prover, base["n"] if n is None else n, n_wires or base["n_wires"], coeffs if coeffs_ is None else coeffs_, mats_)

    def set_(m, k, i, v):
        def f(mats):
            mats[m][k][i] = v
        return f
    refused(r"matrix B row 0: row_ptr starts at 1, not 0", patch=set_(1, 0, 0, 1))
    rp = base["mats"][2][0]
    j = int(np.nonzero(rp[:-1] >= 1)[0][0])               # a row of C that starts past 0: its end is put in front of its start
    refused(r"matrix C row %d: row_ptr decreases" % j, patch=set_(2, 0, j + 1, int(rp[j]) - 1))
    row_of = lambda m, t: int(np.searchsorted(base["mats"][m][0], t, side="right") - 1)
    refused(r"matrix A row %d: wire %d >= n_wires %d" % (row_of(0, 3), base["n_wires"], base["n_wires"]), patch=set_(0, 1, 3, base["n_wires"]))
    refused(r"matrix C row %d: coefficient index %d >= n_coeffs %d" % (row_of(2, 2), len(base["coeffs"]), len(base["coeffs"])),
            patch=set_(2, 2, 2, len(base["coeffs"])))
    k = int(base["mats"][1][2][1])
    first = next((m, row_of(m, int(np.nonzero(base["mats"][m][2] == k)[0][0]))) for m in range(3) if (base["mats"][m][2] == k).any())
    bad = coeffs.copy()
    bad[k] = RC.limbs4([R])[0]
    refused(r"matrix %s row %d: coefficient %d is not canonical" % ("ABC"[first[0]], first[1], k), coeffs_=bad)
    extra = np.concatenate([coeffs, RC.limbs4([2**256 - 1])])
    refused(r"coefficient %d is not canonical \(>= r\); no term uses it" % len(base["coeffs"]), coeffs_=extra)
    empty = [(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))] * 3
    refused(r"n_constraints 0 out of range", n=0, mats=empty)
    refused(r"n_constraints %d out of range" % ((1 << 28) + 1), n=(1 << 28) + 1, mats=empty)   # refused before any array is read
    # NULL arrays with a non-zero count
    lib = prover.lib
    desc, keep = cp.r1cs_desc(base["n"], base["n_wires"], coeffs, base["mats"])
    desc.b.col = None
    assert not lib.cp_r1cs_bls12381_create(prover.ctx, ctypes.byref(desc))
    assert b"matrix B: col / coeff is NULL with %d terms" % len(base["mats"][1][1]) in lib.cp_last_error(None)
    desc, keep = cp.r1cs_desc(base["n"], base["n_wires"], coeffs, base["mats"])
    desc.coeffs = None
    assert not lib.cp_r1cs_bls12381_create(prover.ctx, ctypes.byref(desc))
    assert b"coeffs is NULL with n_coeffs = %d" % len(base["coeffs"]) in lib.cp_last_error(None)
    desc, keep = cp.r1cs_desc(base["n"], base["n_wires"], coeffs, base["mats"])
    desc.a.row_ptr = None
    assert not lib.cp_r1cs_bls12381_create(prover.ctx, ctypes.byref(desc))
    assert b"matrix A: row_ptr is NULL" in lib.cp_last_error(None)
    assert not lib.cp_r1cs_bls12381_create(prover.ctx, None)
    assert b"desc is NULL" in lib.cp_last_error(None)
    # and the unchanged system is accepted
    ok = cp.R1cs(prover, base["n"], base["n_wires"], coeffs, base["mats"])
    ok.free()
