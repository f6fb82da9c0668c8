"""The device's STARK prover and verifier against the DEFINITION of a constraint (tests/air_semantics.py: Python integers, row by
row - checked on the CPU by tests/test_air_semantics.py), not only against the oracle's bytes: the probe AIR has one column per
question a selector answers, and its corruption list sits on the edges the selectors exist for (the wrap from row n - 1 to row
0, a first-row column wrong at row 1, a last-row column wrong at row n - 2, a NEXT load in an every-row constraint). All traces
of one shape are proved in ONE cp_stark_prove_batch call; cp_stark_verify must accept exactly the traces without a violation.
quotient_degree_bits = 0 (one entry of 1 / Z_H, one chunk, the first coset of the LDE at stride 2^rate_bits) is among the shapes
and has parity tests of its own. A map step that loads a column it also stores is refused (the test IS the refusal: such a
program is never run). Every comparison is equality of bytes, of 64-bit words, or of an accept / refuse verdict."""
import ctypes
import os

import numpy as np
import pytest

import air_programs as A
import air_semantics as S
import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
SHAPES = [(3, 0, 1), (4, 0, 1), (4, 1, 1), (5, 0, 2), (5, 2, 2)]   # (degree_bits, quotient_degree_bits, rate_bits)
CASES = [(db, q, rb, top, na) for (db, q, rb) in SHAPES for top in (False, True) for na in (1, 3)]
REFUSAL = "quotient identity fails at zeta"


def fri_of(db, rb):
    return (db, rb, 1, 3, 5, (1,))


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    yield p
    O.lib().or_set_threads(1)
    p.close()


@pytest.fixture(scope="module")
def prover_one_segment():
    """a second context whose interpreter launches are never cut: every program runs as ONE segment"""
    import cityprover
    p = cityprover.Prover(0)
    p.set_option("AIR_TARGET_WAVES", 1)
    yield p
    p.close()


# ---- the probe matrix: inputs and the oracle's side, once per case -------------------------------------------------------------
_cases = {}


def probe_case(db, q, rb, top, na):
    """builder, the 38 instances (honest, then the corruption list) with their publics, the verdict of the definition, and the
    oracle's proof and outgoing challenger of every instance"""
    key = (db, q, rb, top, na)
    if key not in _cases:
        b = S.probe_air(q, db, top)
        trace, pub, glo = S.honest_trace(db, 700 + db)
        cor = S.corruptions(trace, pub)
        assert len(cor) == S.N_CORRUPTIONS == 37          # 7 columns x 5 rows + 2 publics: no case drops out silently
        inst = [("honest", trace, pub)] + [(name, t, pb) for name, _, _, t, pb in cor]
        od, keep = O.stark_desc(db, q, na, O.fri_params(*fri_of(db, rb)), S.N_COLUMNS, b.oracle(), n_public=S.N_PUBLIC, n_global=S.N_GLOBAL)
        want, ok = [], []
        for name, t, pb in inst:
            oc = O.challenger_new()
            O.challenger_observe(oc, [db, q, na])
            want.append((O.stark_prove(od, t, oc, publics=pb, globals_=glo), O.challenger_tuple(oc)))
            ok.append(not S.violations(b, t, pb, glo)[0])
        assert ok.count(True) == 10 and ok[0]            # honest; c1 at n - 1; c2 off row 0; c3 off row n - 1
        _cases[key] = dict(b=b, inst=inst, glo=glo, od=od, keep=keep, want=want, ok=ok, prefix=[db, q, na])
    return _cases[key]


def gpu_desc(p, c, db, q, rb, na):
    import cityprover
    g = c["b"].gpu(p)
    gd, keep = cityprover.stark_desc(db, q, na, cityprover.fri_params(*fri_of(db, rb)), S.N_COLUMNS, g, n_public=S.N_PUBLIC, n_global=S.N_GLOBAL)
    return gd, keep, g


def prove_all_in_one_call(p, c, gd):
    import cityprover
    inst = c["inst"]
    assert len(inst) < cityprover.STARK_BATCH_MAX
    chs = [cityprover.ChallengerState().observe(c["prefix"]) for _ in inst]
    pubs = np.array([pb for _, _, pb in inst], dtype=np.uint64)
    globs = np.array([c["glo"]] * len(inst), dtype=np.uint64)
    got = cityprover.stark_prove_batch(p, gd, [t for _, t, _ in inst], chs, publics=pubs, globals_=globs)
    return got, [x.as_tuple() for x in chs]


@pytest.mark.parametrize("db,q,rb,top,na", CASES)
def test_probe_matrix_one_batch_call_verdicts_follow_the_definition(prover, db, q, rb, top, na):
    import cityprover
    c = probe_case(db, q, rb, top, na)
    gd, keep, g = gpu_desc(prover, c, db, q, rb, na)
    try:
        got, chs = prove_all_in_one_call(prover, c, gd)
        assert len(got) == 38
        refused = 0
        for i, (name, t, pb) in enumerate(c["inst"]):
            assert got[i] == c["want"][i][0], name              # the oracle's bytes, instance by instance
            assert chs[i] == c["want"][i][1], name
            v = cityprover.ChallengerState().observe(c["prefix"])
            if c["ok"][i]:
                cityprover.stark_verify(gd, v, got[i], publics=pb, globals_=c["glo"])
                assert v.as_tuple() == chs[i], name
            else:
                with pytest.raises(cityprover.CityProverError, match=REFUSAL):
                    cityprover.stark_verify(gd, v, got[i], publics=pb, globals_=c["glo"])
                refused += 1
            w = O.challenger_new()
            O.challenger_observe(w, c["prefix"])
            assert O.stark_verify(c["od"], w, got[i], publics=pb, globals_=c["glo"]) == (0 if c["ok"][i] else 2), name
        assert refused == 28
        # the wrong-public instances carry the honest trace (the same trace cap) and are refused all the same
        assert got[36][:80] == got[0][:80] and got[37][:80] == got[0][:80] and got[36] != got[0]
    finally:
        g.close()


@pytest.mark.parametrize("db,q,rb,top,na", CASES)
def test_probe_single_calls_equal_their_batch_instance(prover, db, q, rb, top, na):
    """the honest trace and three corruptions (one accepted: c1 at row n - 1; the wrap row of c4; a wrong public) through
    cp_stark_prove alone"""
    import cityprover
    c = probe_case(db, q, rb, top, na)
    names = [name for name, _, _ in c["inst"]]
    n = 1 << db
    picks = [0, names.index("c1@%d" % (n - 1)), names.index("c4@%d" % (n - 1)), names.index("public1")]
    assert [c["ok"][i] for i in picks] == [True, True, False, False]
    gd, keep, g = gpu_desc(prover, c, db, q, rb, na)
    try:
        batch, batch_chs = prove_all_in_one_call(prover, c, gd)
        for i in picks:
            name, t, pb = c["inst"][i]
            gc = cityprover.ChallengerState().observe(c["prefix"])
            got = cityprover.stark_prove(prover, gd, t, gc, publics=pb, globals_=c["glo"])
            assert got == batch[i] and gc.as_tuple() == batch_chs[i], name
    finally:
        g.close()


@pytest.mark.parametrize("db,q,rb,top,na", CASES)
def test_probe_bytes_do_not_depend_on_the_cut_of_the_interpreter(prover, prover_one_segment, db, q, rb, top, na):
    c = probe_case(db, q, rb, top, na)
    out = []
    for p in (prover, prover_one_segment):
        gd, keep, g = gpu_desc(p, c, db, q, rb, na)
        try:
            assert g.info()["n_segments_max"] == 9
            out.append(prove_all_in_one_call(p, c, gd))
        finally:
            g.close()
    assert out[0] == out[1]
    assert out[0][0] == [w for w, _ in c["want"]]


@pytest.mark.parametrize("top", [False, True])
@pytest.mark.parametrize("db,q,rb", SHAPES)
def test_quotient_of_the_honest_probe_trace_keeps_the_degree_bound(prover, db, q, rb, top):
    """every coefficient above max_k(d_k (n - 1) + e_k) - n is zero, the one AT the bound is not (tests/test_air_semantics.py
    checks the same of the oracle, and that one corruption breaks it)"""
    import cityprover
    n, M = 1 << db, 1 << (db + q)
    b = S.probe_air(q, db, top)
    trace, pub, glo = S.honest_trace(db, 700 + db)
    viol, degrees = S.violations(b, trace, pub, glo)
    assert not viol
    bound = S.quotient_degree_bound(degrees, [k for _, k, _ in S.PROBE_SINKS], n)
    assert bound == (M - (1 << q) if top else n - 2)
    alphas = np.random.default_rng(5).integers(1, P, 3, dtype=np.uint64)
    g = b.gpu(prover)
    T = cityprover.PolyBatch(prover, trace, rb, 1)
    ob = O.Batch(trace, rb, 1)
    try:
        Q = cityprover.air_quotient_commit(prover, g, [T], q, alphas, publics=pub, globals_=glo)
        try:
            raw = Q.coeffs()
        finally:
            Q.close()
        assert (raw == O.air_quotient(b.oracle(), [ob], q, alphas, pub, glo)).all()
        got = raw.reshape(3, M)                          # the 2^q chunks of n of one alpha are consecutive
        assert not got[:, bound + 1:].any()
        assert got[:, bound].all()
    finally:
        g.close()
        T.close()
        ob.close()


# ---- quotient_degree_bits = 0 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_quotient_commit_at_q_0_on_random_degree_2_programs(prover, seed):
    rng = np.random.default_rng(4100 + seed)
    db, rb = (2, 8, 3, 5, 6, 7)[seed], 1 + seed % 3     # 4 .. 256 rows (shorter than a wave included), rates 2 .. 8
    ks = [int(rng.integers(1, 6)) for _ in range(int(rng.integers(1, 4)))]
    b = A.random_program(4200 + seed, sum(ks), int(rng.integers(30, 500)), n_public=seed % 3, n_global=(seed + 1) % 3, n_challenge=seed % 4, max_degree=2)
    info = A.quotient_case(prover, b, ks, db, rb, 0, 1 + seed % 4, int(rng.integers(0, min(db + rb, 4) + 1)), seed)
    assert info["max_constraint_degree"] <= 2


def test_quotient_commit_at_q_0_on_a_gadget_program_at_2_10_rows(prover):
    b = A.gadget_program(4300, 64 + 64, 2000, max_degree=2)
    info = A.quotient_case(prover, b, [64, 64], 10, 1, 0, 2, 4, 4300)
    assert info["n_ops"] >= 2000 and info["max_constraint_degree"] <= 2 and info["n_constraints"] > 50


def extended_descs(p, db, rb, top, map_builder=None):
    """the probe with one extended column at q = 0 (every sink has degree <= 2): its map step reads trace columns only"""
    import cityprover
    b, m = S.probe_air(0, db, top, extended=True), map_builder or S.probe_map()
    gp = [b.gpu(p), m.gpu(p)]
    gd, gk = cityprover.stark_desc(db, 0, 2, cityprover.fri_params(*fri_of(db, rb)), S.N_COLUMNS, gp[0], 1, 1, n_public=S.N_PUBLIC, n_global=S.N_GLOBAL,
                                   steps=[("map", gp[1])])
    od, ok = O.stark_desc(db, 0, 2, O.fri_params(*fri_of(db, rb)), S.N_COLUMNS, b.oracle(), 1, 1, n_public=S.N_PUBLIC, n_global=S.N_GLOBAL,
                          steps=[("map", m.oracle())])
    return gd, od, (gk, ok), gp


@pytest.mark.parametrize("db,rb,top", [(3, 1, True), (5, 2, False), (7, 1, True)])
def test_whole_prover_at_q_0_with_an_extended_column(prover, db, rb, top):
    import cityprover
    gd, od, keep, gp = extended_descs(prover, db, rb, top)
    trace, pub, glo = S.honest_trace(db, 900 + db)
    bad = trace.copy()
    bad[0, 1] = 1
    try:
        for t, rc in ((trace, 0), (bad, 2)):
            oc, gc = O.challenger_new(), cityprover.ChallengerState()
            want = O.stark_prove(od, t, oc, publics=pub, globals_=glo)
            got = cityprover.stark_prove(prover, gd, t, gc, publics=pub, globals_=glo)
            assert got == want and gc.as_tuple() == O.challenger_tuple(oc)
            assert O.stark_verify(od, O.challenger_new(), got, publics=pub, globals_=glo) == rc
            if rc == 0:
                cityprover.stark_verify(gd, cityprover.ChallengerState(), got, publics=pub, globals_=glo)
            else:
                with pytest.raises(cityprover.CityProverError, match=REFUSAL):
                    cityprover.stark_verify(gd, cityprover.ChallengerState(), got, publics=pub, globals_=glo)
        both = cityprover.stark_prove_batch(prover, gd, [trace, bad], [cityprover.ChallengerState(), cityprover.ChallengerState()],
                                            publics=np.array([pub, pub], dtype=np.uint64), globals_=np.array([glo, glo], dtype=np.uint64))
        assert both[1] == got and both[0] != got
    finally:
        for g in gp:
            g.close()


# ---- a map step that loads what it stores -----------------------------------------------------------------------------------
def self_reading_map(kind):
    """extended column 0 <- itself (this row / the next row) + c7: input column 8 IS output column 0 in a STARK step"""
    m = A.Builder(A.MAP, S.N_COLUMNS + 1, S.N_PUBLIC, S.N_GLOBAL, 1, n_out_columns=1)
    own = m.local(S.N_COLUMNS) if kind == "local" else m.next(S.N_COLUMNS)
    m.store(0, m.add(own, m.local(7)))
    return m


@pytest.mark.parametrize("kind", ["local", "next"])
def test_a_map_step_that_loads_what_it_stores_is_refused(prover, kind):
    import cityprover
    db, rb = 4, 1
    lib = prover.lib
    trace, pub, glo = S.honest_trace(db, 900 + db)
    good_gd, od, good_keep, good_gp = extended_descs(prover, db, rb, False)
    gd, _, keep, gp = extended_descs(prover, db, rb, False, self_reading_map(kind))
    message = r"step 0: the map program loads extended column 0, which it also stores"
    try:
        oc = O.challenger_new()
        O.challenger_observe(oc, [5, 6])
        want = O.stark_prove(od, trace, oc, publics=pub, globals_=glo)
        gc = cityprover.ChallengerState().observe([5, 6])
        assert cityprover.stark_prove(prover, good_gd, trace, gc, publics=pub, globals_=glo) == want
        # cp_stark_prove: refused, the transcript untouched, no proof handed out
        gc = cityprover.ChallengerState().observe([5, 6])
        before = gc.as_tuple()
        with pytest.raises(cityprover.CityProverError, match=message):
            cityprover.stark_prove(prover, gd, trace, gc, publics=pub, globals_=glo)
        assert gc.as_tuple() == before
        t = np.ascontiguousarray(trace)
        pp, gg = np.array(pub, dtype=np.uint64), np.array(glo, dtype=np.uint64)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(7)
        assert lib.cp_stark_prove(prover.ctx, ctypes.byref(gd), t.ctypes.data, 0, pp.ctypes.data_as(u64p), gg.ctypes.data_as(u64p), ctypes.byref(gc), 0, 0,
                                  ctypes.byref(out), ctypes.byref(ln)) == -1
        assert not out and ln.value == 0 and gc.as_tuple() == before
        # cp_stark_prove_batch: all or nothing - no challenger moved, no output pointer or length written
        B = 3
        tp = (ctypes.c_void_p * B)(*[t.ctypes.data] * B)
        pubs, globs = np.array([pub] * B, dtype=np.uint64), np.array([glo] * B, dtype=np.uint64)
        chs = (cityprover.ChallengerState * B)()
        for i in range(B):
            x = cityprover.ChallengerState().observe([5, 6, i])
            ctypes.memmove(ctypes.byref(chs[i]), ctypes.byref(x), ctypes.sizeof(x))
        chs_before = bytes(chs)
        outs, lens = (ctypes.POINTER(ctypes.c_uint8) * B)(), (ctypes.c_size_t * B)()
        sentinel = 0x5A5A5A50
        for i in range(B):
            outs[i], lens[i] = ctypes.cast(sentinel, ctypes.POINTER(ctypes.c_uint8)), 7
        rc = lib.cp_stark_prove_batch(prover.ctx, ctypes.byref(gd), B, tp, 0, pubs.ctypes.data_as(u64p), globs.ctypes.data_as(u64p), chs, None, None, outs, lens)
        msg = lib.cp_last_error(prover.ctx).decode()
        assert rc == -1 and message in msg, (rc, msg)
        assert bytes(chs) == chs_before and all(ctypes.cast(outs[i], ctypes.c_void_p).value == sentinel and lens[i] == 7 for i in range(B))
        # the next good call gives its old bytes, alone and in a batch
        gc = cityprover.ChallengerState().observe([5, 6])
        assert cityprover.stark_prove(prover, good_gd, trace, gc, publics=pub, globals_=glo) == want
        assert gc.as_tuple() == O.challenger_tuple(oc)
        two = cityprover.stark_prove_batch(prover, good_gd, [trace, trace], [cityprover.ChallengerState().observe([5, 6]) for _ in range(2)],
                                           publics=pubs[:2], globals_=globs[:2])
        assert two == [want, want]
    finally:
        for g in gp + good_gp:
            g.close()


@pytest.mark.parametrize("kind", ["local", "next"])
def test_air_map_dev_refuses_overlapping_columns_and_runs_disjoint_ones(prover, kind):
    import cityprover
    k0, n = S.N_COLUMNS, 100
    m = self_reading_map(kind)
    g, o = m.gpu(prover), m.oracle()
    rng = np.random.default_rng(12)
    cols = rng.integers(0, P, (k0 + 1, n), dtype=np.uint64)
    pub, glo, cha = (np.array(v, dtype=np.uint64) for v in ([1, 2], [4], [3]))
    u64p = ctypes.POINTER(ctypes.c_uint64)
    d = prover.to_device(cols)
    try:
        # out = in + k0 n: output column 0 is input column k0, which the program loads - refused, and nothing was written
        uni = [x.ctypes.data_as(u64p) for x in (pub, glo, cha)]
        rc = prover.lib.cp_air_map_dev(prover.ctx, g.handle, d.ptr, d.ptr + k0 * n * 8, n, *uni)
        msg = prover.lib.cp_last_error(prover.ctx).decode()
        assert rc == -1 and "the map program loads extended column 0, which it also stores" in msg and "step" not in msg, (rc, msg)
        assert (d.download().reshape(k0 + 1, n) == cols).all()
        # one element of overlap is an overlap
        rc = prover.lib.cp_air_map_dev(prover.ctx, g.handle, d.ptr, d.ptr + (k0 + 1) * n * 8 - 8, n, *uni)
        assert rc == -1 and "which it also stores" in prover.lib.cp_last_error(prover.ctx).decode()
        # the same program with an output array of its own: the oracle's columns
        assert (cityprover.air_map(prover, g, cols, pub, glo, cha) == o.map(cols, pub, glo, cha)).all()
    finally:
        d.free()
        g.close()


def test_a_step_may_load_what_an_earlier_step_stored(prover):
    """the toy lookup AIR: its map B loads the extended columns map A stored and the inversion replaced - still proved, alone and
    in a batch, to the oracle's bytes"""
    import cityprover
    db = 4
    progs = A.lookup_programs()
    gp, op = [x.gpu(prover) for x in progs], [x.oracle() for x in progs]
    gd, gk = cityprover.stark_desc(db, 1, 2, cityprover.fri_params(db, 1, 2, 5, 12, (2,)), A.LOOKUP_K0, gp[0], A.LOOKUP_K1, 3, steps=A.lookup_steps(gp[1], gp[2]))
    od, ok = O.stark_desc(db, 1, 2, O.fri_params(db, 1, 2, 5, 12, (2,)), A.LOOKUP_K0, op[0], A.LOOKUP_K1, 3, steps=A.lookup_steps(op[1], op[2]))
    trace = A.lookup_trace(1 << db)
    try:
        want = O.stark_prove(od, trace, O.challenger_new())
        assert cityprover.stark_prove(prover, gd, trace, cityprover.ChallengerState()) == want
        assert cityprover.stark_prove_batch(prover, gd, [trace, trace], [cityprover.ChallengerState(), cityprover.ChallengerState()]) == [want, want]
        cityprover.stark_verify(gd, cityprover.ChallengerState(), want)
    finally:
        for g in gp:
            g.close()
