"""GPU: cp_air_check_rows_dev / cp_stark_check_trace against the DEFINITION of a constraint (tests/air_semantics.py: Python
integers, row by row): the count of (row, sink) pairs where a sink that binds the row is not zero, the first of them in the
order row, then sink, with its kind and value, and the count per sink.

The probe AIR at 2^3 rows (first, second, middle, n - 2 and n - 1 within one wave), 2^5 and 2^8 rows (several blocks at two rows
per lane): the honest trace - which breaks every sink on the rows that sink does NOT bind - and the 37 corruptions of
air_semantics.corruptions. The probe with its extended column through cp_stark_check_trace under two round challenges. Programs
that run as many segments (one block per segment): a chain AIR whose trace satisfies it, corrupted so that sinks of different
segments break on one row and a third on an earlier row of another block, and a seeded random program of air_programs.py on a
random trace, both also as ONE segment. The SHA-256 AIR at its smallest message. The refusals. Every comparison is an equality."""
import collections
import ctypes

import numpy as np
import pytest

import air_programs as A
import air_semantics as S
import sha256_air as SHA

pytestmark = pytest.mark.gpu
P = A.P


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def prover_one_segment():
    """a second context whose interpreter launches are never cut: every program runs as ONE segment"""
    import cityprover
    p = cityprover.Prover(0)
    p.set_option("AIR_TARGET_WAVES", 1)
    yield p
    p.close()


def expected_report(builder, trace, publics=(), globals_=(), challenges=()):
    """the report the definition gives: from air_semantics.violations and sink_values"""
    viol, _ = S.violations(builder, trace, publics, globals_, challenges)
    values, kinds, _ = S.sink_values(builder, trace, publics, globals_, challenges)
    tally = collections.Counter(k for k, _, _ in viol)
    rep = dict(n_violations=len(viol), row=-1, sink=-1, sink_kind=-1, value=0, per_sink=[tally[k] for k in range(len(kinds))])
    if viol:
        k, kind, r = min(viol, key=lambda v: (v[2], v[0]))
        rep.update(row=r, sink=k, sink_kind=A.SINKS[kind], value=values[k][r])
    return rep


# ---- the probe AIR -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("db", [3, 5, 8])
def test_probe_air_honest_trace_and_every_corruption(prover, db):
    n = 1 << db
    b = S.probe_air(1, db)
    trace, pub, glo = S.honest_trace(db, 700 + db)
    cor = S.corruptions(trace, pub)
    assert len(cor) == S.N_CORRUPTIONS == 37
    # the list the definition computes must agree with the hand-written table, before the device is asked anything
    for name, col, row, t, pb in cor:
        assert S.violations(b, t, pb, glo)[0] == S.expected_violations(col, row, n, name), name
    values, kinds, _ = S.sink_values(b, trace, pub, glo)
    assert all(any(values[k][r] for r in range(n) if not S.binds(kinds[k], r, n)) for k in range(len(kinds)) if kinds[k] != "all")
    g = b.gpu(prover)
    try:
        honest = g.check_rows(trace, pub, glo)
        assert honest == dict(n_violations=0, row=-1, sink=-1, sink_kind=-1, value=0, per_sink=[0] * 9)
        n_ok = 0
        for name, col, row, t, pb in cor:
            exp = S.expected_violations(col, row, n, name)
            got = g.check_rows(t, pb, glo)
            assert got["n_violations"] == len(exp), name
            if exp:
                k, kind, r = min(exp, key=lambda v: (v[2], v[0]))
                vals = S.sink_values(b, t, pb, glo)[0]
                assert (got["row"], got["sink"], got["sink_kind"], got["value"]) == (r, k, A.SINKS[kind], vals[k][r]), name
            else:
                assert (got["row"], got["sink"], got["sink_kind"], got["value"]) == (-1, -1, -1, 0), name
                n_ok += 1
            tally = collections.Counter(k for k, _, _ in exp)
            assert got["per_sink"] == [tally[k] for k in range(9)], name
            assert got == expected_report(b, t, pb, glo), name
        assert n_ok == 9        # c1 at n - 1; c2 off row 0; c3 off row n - 1
    finally:
        g.close()


def fri_of(db, rb):
    return (db, rb, 1, 3, 5, (1,))


@pytest.mark.parametrize("db", [3, 7])
def test_probe_with_an_extended_column_through_stark_check_trace(prover, db):
    import cityprover as cp
    n = 1 << db
    b, m = S.probe_air(0, db, extended=True), S.probe_map()
    gp = [b.gpu(prover), m.gpu(prover)]
    gd, keep = cp.stark_desc(db, 0, 2, cp.fri_params(*fri_of(db, 1)), S.N_COLUMNS, gp[0], 1, 1, n_public=S.N_PUBLIC, n_global=S.N_GLOBAL,
                             steps=[("map", gp[1])])
    trace, pub, glo = S.honest_trace(db, 900 + db)

    def extended(t, ch):      # the definition of the map step: challenge0 * c7 + next(c4)
        return np.array([(ch * int(t[7, r]) + int(t[4, (r + 1) % n])) % P for r in range(n)], dtype=np.uint64)

    bad = trace.copy()
    r0 = n // 2
    bad[4, r0] = (int(bad[4, r0]) + 1) % P
    try:
        for ch in (3, 0x1234567890ABCDEF % P):
            rep = cp.stark_check_trace(prover, gd, trace, pub, glo, [ch], n_constraints=10)
            assert rep == dict(n_violations=0, row=-1, sink=-1, sink_kind=-1, value=0, per_sink=[0] * 10)
            # the extended column is filled from the trace that is checked: a corrupted c4 breaks its own sink on the two rows that read it
            full = np.vstack([bad, extended(bad, ch)[None]])
            want = expected_report(b, full, pub, glo, [ch])
            assert want["per_sink"] == [0, 0, 0, 0, 2, 0, 0, 0, 0, 0] and (want["row"], want["sink"]) == (r0 - 1, 4)
            assert cp.stark_check_trace(prover, gd, bad, pub, glo, [ch], n_constraints=10) == want
            assert cp.stark_check_trace(prover, gd, bad, pub, glo, [ch])["per_sink"] == []       # per_sink_out may be NULL
            # an extended column that was filled from ANOTHER trace (the honest one): sinks 4 and 9 on the rows that read the cell
            stale = np.vstack([bad, extended(trace, ch)[None]])
            want = expected_report(b, stale, pub, glo, [ch])
            assert want["per_sink"] == [0, 0, 0, 0, 2, 0, 0, 0, 0, 1] and (want["row"], want["sink"]) == (r0 - 1, 4)
            assert gp[0].check_rows(stale, pub, glo, [ch]) == want
    finally:
        for g in gp:
            g.close()


# ---- programs in several segments --------------------------------------------------------------------------------------------
CHAIN_COLUMNS = 96


def chain_air(seed):
    """next(c_j) = c_j c_(j+1) + k_j on rows 0 .. n - 2, one transition sink per column: 96 independent sinks, cut into as many
    segments as the launch wants; and the trace the recurrence gives from a seeded first row"""
    rng = np.random.default_rng(seed)
    ks = [int(v) for v in rng.integers(1, P, CHAIN_COLUMNS, dtype=np.uint64)]
    b = A.Builder(A.CONSTRAINTS, CHAIN_COLUMNS)
    for j in range(CHAIN_COLUMNS):
        b.assert_zero(b.sub(b.next(j), b.add(b.mul(b.local(j), b.local((j + 1) % CHAIN_COLUMNS)), b.const(ks[j]))), "transition")
    return b, ks, [int(v) for v in rng.integers(0, P, CHAIN_COLUMNS, dtype=np.uint64)]


def chain_trace(ks, first_row, n):
    t = np.zeros((CHAIN_COLUMNS, n), dtype=np.uint64)
    row = list(first_row)
    for r in range(n):
        t[:, r] = np.array(row, dtype=np.uint64)
        row = [(row[j] * row[(j + 1) % CHAIN_COLUMNS] + ks[j]) % P for j in range(CHAIN_COLUMNS)]
    return t


def test_sinks_of_different_segments_on_one_row_and_an_earlier_row_in_another_block(prover, prover_one_segment):
    n = 256
    b, ks, first = chain_air(31)
    trace = chain_trace(ks, first, n)
    assert expected_report(b, trace)["n_violations"] == 0          # the wrap row breaks every sink and binds none
    bad = trace.copy()
    for col, row in ((10, 200), (70, 200), (40, 50)):
        bad[col, row] = (int(bad[col, row]) + 1) % P
    want = expected_report(b, bad)
    # a cell is read by its own sink on its row and the row before, and by the sink of the column before it on its row
    assert want["n_violations"] == 9 and (want["row"], want["sink"]) == (49, 40)
    assert [k for k, c in enumerate(want["per_sink"]) if c] == [9, 10, 39, 40, 69, 70]
    two = bad.copy()
    two[40, 50] = trace[40, 50]
    want_two = expected_report(b, two)
    assert (want_two["row"], want_two["sink"], want_two["n_violations"]) == (199, 10, 6)      # one row, sinks of two segments: the lowest
    for p in (prover, prover_one_segment):
        g = b.gpu(p)
        try:
            assert g.info()["n_segments_max"] == CHAIN_COLUMNS > 1
            assert g.check_rows(trace)["n_violations"] == 0
            assert g.check_rows(bad) == want
            assert g.check_rows(two) == want_two
        finally:
            g.close()


@pytest.mark.parametrize("seed,n_columns,n_ops,log_rows", [(5, 12, 300, 6), (6, 40, 1500, 8), (7, 9, 120, 2)])
def test_seeded_random_program_on_a_random_trace(prover, prover_one_segment, seed, n_columns, n_ops, log_rows):
    """nearly every sink breaks on nearly every row it binds: the counts per sink are the numbers of rows each kind binds, less the
    zeros the definition finds"""
    rng = np.random.default_rng(8000 + seed)
    b = A.random_program(seed, n_columns, n_ops, max_degree=3)
    n = 1 << log_rows
    trace = rng.integers(0, P, (n_columns, n), dtype=np.uint64)
    trace[:, n // 2] = 0            # and some rows of zeros and ones, where products vanish
    trace[:, n - 1] = 1
    pub, glo, cha = ([int(v) for v in rng.integers(0, P, k, dtype=np.uint64)] for k in (b.n_public, b.n_global, b.n_challenge))
    want = expected_report(b, trace, pub, glo, cha)
    assert want["n_violations"] > n and len(want["per_sink"]) > 1
    for p in (prover, prover_one_segment):
        g = b.gpu(p)
        try:
            assert g.info()["n_segments_max"] > 1
            assert g.check_rows(trace, pub, glo, cha) == want
        finally:
            g.close()


# ---- SHA-256 -----------------------------------------------------------------------------------------------------------------
def test_sha256_air_at_its_smallest_message(prover):
    log_rows = 7
    t, digest = SHA.check(SHA.random_message(3, log_rows), log_rows)
    g = SHA.program().gpu(prover)
    try:
        n_sinks = g.info()["n_constraints"]
        honest = g.check_rows(t, digest)
        assert honest == dict(n_violations=0, row=-1, sink=-1, sink_kind=-1, value=0, per_sink=[0] * n_sinks)
        row = 40
        bad = t.copy()
        bad[SHA.X0 + 32 * 4 + 3, row] ^= 1        # one bit of e before round 40
        rep = g.check_rows(bad, digest)
        assert rep["n_violations"] > 0 and rep["row"] in (row - 1, row)
        assert rep["n_violations"] == sum(rep["per_sink"]) and rep["per_sink"][rep["sink"]] >= 1 and rep["value"] != 0
        assert not any(rep["per_sink"][:rep["sink"]]) or rep["row"] == row - 1      # the lowest sink of the first row
    finally:
        g.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(prover):
    import cityprover as cp
    db = 4
    n = 1 << db
    b, m = S.probe_air(0, db, extended=True), S.probe_map()
    plain = S.probe_air(1, db)
    gp = [b.gpu(prover), m.gpu(prover), plain.gpu(prover)]
    gd, keep = cp.stark_desc(db, 0, 2, cp.fri_params(*fri_of(db, 1)), S.N_COLUMNS, gp[0], 1, 1, n_public=S.N_PUBLIC, n_global=S.N_GLOBAL,
                             steps=[("map", gp[1])])
    trace, pub, glo = S.honest_trace(db, 900 + db)
    lib = prover.lib
    u64p = ctypes.POINTER(ctypes.c_uint64)
    pp, gg = np.array(pub, dtype=np.uint64), np.array(glo, dtype=np.uint64)
    d = prover.to_device(trace)

    def usable():
        assert gp[2].check_rows(trace, pub, glo)["n_violations"] == 0
        assert cp.stark_check_trace(prover, gd, trace, pub, glo, [5])["n_violations"] == 0

    try:
        with pytest.raises(cp.CityProverError, match="not a CP_AIR_CONSTRAINTS program"):
            gp[1].check_rows(np.vstack([trace, trace[:1]]), pub, glo, [5])
        usable()
        with pytest.raises(cp.CityProverError, match="n = 12 is not a power of two"):
            gp[2].check_rows(trace[:, :12], pub, glo)
        usable()
        with pytest.raises(cp.CityProverError, match="not canonical"):
            gp[2].check_rows(trace, (P, pub[1]), glo)
        usable()
        rep = cp.AirCheckReport()
        args = (pp.ctypes.data_as(u64p), gg.ctypes.data_as(u64p), None)
        assert lib.cp_air_check_rows_dev(prover.ctx, gp[2].handle, d.ptr, n, *args, None, None) == -1
        assert b"NULL argument" in lib.cp_last_error(prover.ctx)
        assert lib.cp_air_check_rows_dev(prover.ctx, None, d.ptr, n, *args, ctypes.byref(rep), None) == -1
        assert b"NULL argument" in lib.cp_last_error(prover.ctx)
        assert lib.cp_air_check_rows_dev(prover.ctx, gp[2].handle, None, n, *args, ctypes.byref(rep), None) == -1
        assert b"NULL column array" in lib.cp_last_error(prover.ctx)
        assert lib.cp_air_check_rows_dev(prover.ctx, gp[2].handle, d.ptr, n, None, args[1], None, ctypes.byref(rep), None) == -1
        assert b"NULL publics" in lib.cp_last_error(prover.ctx)
        usable()
        # cp_stark_check_trace: NULL description / trace / report, missing round challenges, a trace element >= p
        t = np.ascontiguousarray(trace)
        assert lib.cp_stark_check_trace(prover.ctx, None, t.ctypes.data, 0, *args, ctypes.byref(rep), None) == -1
        assert b"desc is NULL" in lib.cp_last_error(prover.ctx)
        assert lib.cp_stark_check_trace(prover.ctx, ctypes.byref(gd), None, 0, *args, ctypes.byref(rep), None) == -1
        assert lib.cp_stark_check_trace(prover.ctx, ctypes.byref(gd), t.ctypes.data, 0, *args, None, None) == -1
        assert lib.cp_stark_check_trace(prover.ctx, ctypes.byref(gd), t.ctypes.data, 0, *args, ctypes.byref(rep), None) == -1
        assert b"round challenges" in lib.cp_last_error(prover.ctx)
        with pytest.raises(cp.CityProverError, match="round challenge is not canonical"):
            cp.stark_check_trace(prover, gd, trace, pub, glo, [P])
        over = trace.copy()
        over[5, 9] = P
        with pytest.raises(cp.CityProverError, match="a trace value is not canonical"):
            cp.stark_check_trace(prover, gd, over, pub, glo, [5])
        assert bytes(rep) == bytes(ctypes.sizeof(rep))        # no refusal wrote the report
        usable()
    finally:
        d.free()
        for g in gp:
            g.close()
