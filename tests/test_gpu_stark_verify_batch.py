"""cp_stark_verify_batch (include/cityprover.h): B STARK proofs of one description in one call, the query phase on the device. The
contract is the verdict of cp_stark_verify, proof by proof - its first failure, in its own order - and its outgoing challenger
for the accepted ones, under each of the three path forms: one lane per path (friv::k_paths), twelve lanes per path
(friv::k_paths_coop) and the library's choice. Proofs come from cp_stark_prove_batch. The shapes are the smallest at which the
twelve-lane kernel takes another path: every case of the leaf sponge, paths of depth 0, partly filled waves and workgroups, an
inactive proof inside a wave. The GPU is touched only inside tests."""
import ctypes

import numpy as np
import pytest

import air_programs as A
import oracle_lib as O
import stark_proof_words as W
from test_gpu_alloc_faults import walk
from test_gpu_stark_batch import CHEATS, gpu_batch, launches_of, toy_instance

pytestmark = pytest.mark.gpu
P = O.P
FORMS = (1, 2, 0)   # cityprover.PATHS_LANE, PATHS_COOP, PATHS_AUTO
OK = W.OK


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def batch(p, gd, proofs, prefixes, form, pubs=None, globs=None, chunk=0):
    """one call -> (verdict triples, outgoing challengers, incoming challengers)"""
    import cityprover
    chs = [W.challenger(pre) for pre in prefixes]
    before = [c.as_tuple() for c in chs]
    got = cityprover.stark_verify_batch(p, gd, chs, proofs, publics=pubs, globals_=globs, chunk=chunk, path_form=form)
    return got, [c.as_tuple() for c in chs], before


def host_all(gd, proofs, prefixes, pubs=None, globs=None):
    return [W.host_verdict(gd, prefixes[i], proofs[i], None if pubs is None else pubs[i], None if globs is None else globs[i]) for i in range(len(proofs))]


def assert_as_host(p, gd, proofs, prefixes, want, pubs=None, globs=None, chunk=0, forms=FORMS):
    """under every form: the host verifier's verdict, its challenger for an accepted proof, the incoming one for a rejected proof"""
    for form in forms:
        got, after, before = batch(p, gd, proofs, prefixes, form, pubs, globs, chunk)
        for i, (v, ch) in enumerate(want):
            assert got[i] == v, (form, i, got[i], v)
            assert after[i] == (ch if v == OK else before[i]), (form, i)


# ---- 1. the toy AIR with a lookup: agreement with the host verifier, proof by proof ------------------------------------------
def toy_descs(p, db, nq=12, pow_bits=5, arity=(2,), ch=2):
    """(gpu desc, oracle desc, keep-alives, gpu programs to close, the layout's arguments)"""
    import cityprover
    progs = A.lookup_programs()
    gp = [x.gpu(p) for x in progs]
    op = [x.oracle() for x in progs]
    gd, gk = cityprover.stark_desc(db, 1, 2, cityprover.fri_params(db, 1, ch, pow_bits, nq, arity), A.LOOKUP_K0, gp[0], A.LOOKUP_K1, 3,
                                   steps=A.lookup_steps(gp[1], gp[2]))
    od, ok = O.stark_desc(db, 1, 2, O.fri_params(db, 1, ch, pow_bits, nq, arity), A.LOOKUP_K0, op[0], A.LOOKUP_K1, 3, steps=A.lookup_steps(op[1], op[2]))
    return gd, od, (gk, ok, op), gp, (db, 1, ch, nq, arity, A.LOOKUP_K0, A.LOOKUP_K1, 2 << 1)


def close(progs):
    for g in progs:
        g.close()


@pytest.mark.parametrize("db", [4, 7])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_toy_air_verdicts_equal_the_host_verifier_proof_by_proof(prover, db, B):
    gd, od, keep, gp, _ = toy_descs(prover, db)
    try:
        inst = [toy_instance(i, db) for i in range(B)]   # honest, a looked-up value outside the table (with an injected witness), a broken transition, ...
        prefixes = [pre for _, pre, _ in inst]
        proofs, _ = gpu_batch(prover, gd, [t for t, _, _ in inst], prefixes, [w for _, _, w in inst])
        want = host_all(gd, proofs, prefixes)
        for i in range(B):
            assert (want[i][0] == OK) == (CHEATS[i % 3] is None), (i, want[i][0])
            if CHEATS[i % 3] is None:
                oc = O.challenger_new()
                O.challenger_observe(oc, prefixes[i])
                assert O.stark_verify(od, oc, proofs[i]) == 0
                assert O.challenger_tuple(oc) == want[i][1]
            else:
                assert want[i][0][0] == 5
        assert_as_host(prover, gd, proofs, prefixes, want)
    finally:
        close(gp)


# ---- 2. leaf lengths and depths ---------------------------------------------------------------------------------------------
def chained_air(seed, k):
    """A seeded AIR over k columns that a trace can SATISFY (the seeded random programs of air_programs.py are not satisfiable, and
    a refused proof never reaches the kernels): column 0 is a recurrence c0' = c0^2 + a with a given first row (a transition and a
    first-row constraint), column j >= 1 is c_j = c_x c_y + m c_z + e of earlier columns on every row. -> (builder, trace(n))"""
    rng = np.random.default_rng(7000 + seed)
    r = lambda: int(rng.integers(1, P, dtype=np.uint64))
    a, first = r(), r()
    spec = [(int(rng.integers(0, j)), int(rng.integers(0, j)), int(rng.integers(0, j)), r(), r()) for j in range(1, k)]
    b = A.Builder(A.CONSTRAINTS, k)
    c0 = b.local(0)
    b.assert_zero(b.sub(b.next(0), b.add(b.mul(c0, c0), b.const(a))), "transition")
    b.assert_zero(b.sub(b.local(0), b.const(first)), "first")
    for j, (x, y, z, m, e) in enumerate(spec, 1):
        rhs = b.add(b.add(b.mul(b.local(x), b.local(y)), b.mul(b.const(m), b.local(z))), b.const(e))
        b.assert_zero(b.sub(b.local(j), rhs), "all")

    def trace(n):
        t = [[0] * n for _ in range(k)]
        t[0][0] = first
        for i in range(1, n):
            t[0][i] = (t[0][i - 1] * t[0][i - 1] + a) % P
        for j, (x, y, z, m, e) in enumerate(spec, 1):
            t[j] = [(t[x][i] * t[y][i] + m * t[z][i] + e) % P for i in range(n)]
        return np.array(t, dtype=np.uint64)
    return b, trace


# (trace width, FRI arities, cap height or None = the LDE size's log: paths of depth 0, degree_bits, num_challenges). Widths: a leaf
# that is its own digest (1, 3, 4), 5 .. 7 elements with no absorb step (5, 7), exact chunks (8, 16), a partial last chunk with a
# chunk before it that keeps everything (9, 15, 17, 25); the quotient leaf has 2, 4, 6 or 8 elements (num_challenges x 2); layer
# leaves of 4, 8 and 16 elements; a layer path of depth 0 under oracle paths of depth 2 (5, (2,), 2, 3); no layer at all: the final
# polynomial has the full degree.
EDGE_CASES = [(1, (), None, 3, 1), (3, (1,), 0, 3, 2), (4, (2,), 0, 4, 3), (5, (3, 1), 0, 5, 4), (5, (2,), 2, 3, 2), (7, (), 0, 3, 3),
              (8, (1,), 0, 4, 4), (9, (2,), 0, 5, 1), (15, (3, 1), 0, 4, 2), (16, (), None, 4, 3), (17, (2,), 1, 3, 4), (25, (3, 1), 0, 5, 3),
              (9, (), None, 5, 2), (25, (1,), 1, 4, 1)]


@pytest.mark.parametrize("k,arity,ch,db,na", EDGE_CASES)
def test_leaf_length_and_depth_edges_are_accepted_under_every_form(prover, k, arity, ch, db, na):
    import cityprover
    ch = db + 1 if ch is None else ch
    b, trace = chained_air(k, k)
    g = b.gpu(prover)
    try:
        gd, keep = cityprover.stark_desc(db, 1, na, cityprover.fri_params(db, 1, ch, 3, 3, arity), k, g)
        od, okeep = O.stark_desc(db, 1, na, O.fri_params(db, 1, ch, 3, 3, arity), k, b.oracle())
        prefixes = [[1, 2, 3], [4, 5]]
        proofs, _ = gpu_batch(prover, gd, [trace(1 << db)] * 2, prefixes, [None, None])
        assert len(proofs[0]) == 8 * len(W.layout(db, 1, ch, 3, arity, k, 0, na << 1))
        want = host_all(gd, proofs, prefixes)
        assert [v for v, _ in want] == [OK, OK]
        oc = O.challenger_new()
        O.challenger_observe(oc, prefixes[0])
        assert O.stark_verify(od, oc, proofs[0]) == 0
        assert_as_host(prover, gd, proofs, prefixes, want)
        # and a leaf element of every oracle's last round is missed by no form (the last element: the partial chunk where there is one)
        lab = W.layout(db, 1, ch, 3, arity, k, 0, na << 1)
        for o, last in ((0, k - 1), (1, (na << 1) - 1)):
            i = lab.index(("leaf", 2, o, last))
            bad = W.with_words(proofs[1], [(i, (int(W.words_of(proofs[1])[i]) + 1) % P)])
            for form in FORMS:
                assert batch(prover, gd, [proofs[0], bad], prefixes, form)[0] == [OK, (7, 2, o)], (form, o)
    finally:
        g.close()


# ---- 3. group and workgroup boundaries ----------------------------------------------------------------------------------------
def honest_toy_proofs(p, gd, db, B):
    prefixes = [[100 + i, i] for i in range(B)]
    proofs, _ = gpu_batch(p, gd, [A.lookup_trace(1 << db)] * B, prefixes, [None] * B)
    return proofs, prefixes


def last_sibling_words(lab, nq, n_or, n_layers):
    """per tree: (the word of the last limb of the last sibling of the last query round, the verdict a change of it must give)"""
    out = []
    for o in range(n_or):
        idx = [i for i, l in enumerate(lab) if l[:3] == ("sib", nq - 1, o)]
        out.append((idx[-1], (7, nq - 1, o)))
    for l in range(n_layers):
        idx = [i for i, x in enumerate(lab) if x[:3] == ("lsib", nq - 1, l)]
        out.append((idx[-1], (9, nq - 1, l)))
    return out


# paths per tree = B x query rounds: 1, 4, 5, 6 (a partly filled wave, a full one, one group into the next wave), 19, 20, 21 (a partly
# filled workgroup, a full one, one group into the next), 41 (three workgroups)
@pytest.mark.parametrize("B,nq", [(1, 1), (4, 1), (5, 1), (6, 1), (19, 1), (20, 1), (3, 7), (1, 41)])
def test_group_and_workgroup_boundaries(prover, B, nq):
    db = 4
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=nq)
    try:
        proofs, prefixes = honest_toy_proofs(prover, gd, db, B)
        lab = W.layout(*shape)
        victim = B - 1   # its last round is the last path of every tree: the last used group of the last wave
        for word, want in last_sibling_words(lab, nq, 3, 1):
            changed = list(proofs)
            changed[victim] = W.with_words(proofs[victim], [(word, (int(W.words_of(proofs[victim])[word]) + 1) % P)])
            assert W.host_verdict(gd, prefixes[victim], changed[victim])[0] == want
            for form in FORMS:
                got, after, before = batch(prover, gd, changed, prefixes, form)
                assert got == [OK] * victim + [want], (form, want, got)
                assert after[victim] == before[victim] and all(after[i] != before[i] for i in range(victim))
    finally:
        close(gp)


@pytest.mark.parametrize("B,nq,dead,victim", [(6, 1, 2, 3), (3, 7, 1, 2), (7, 3, 3, 2)])
def test_an_inactive_proof_inside_a_wave_disturbs_no_neighbour(prover, B, nq, dead, victim):
    """proof `dead` is cut short, so the host phase has its verdict and its groups carry dummies; its neighbour `victim` has a
    changed sibling, everyone else is accepted"""
    db = 4
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=nq)
    try:
        proofs, prefixes = honest_toy_proofs(prover, gd, db, B)
        lab = W.layout(*shape)
        for word, want in last_sibling_words(lab, nq, 3, 1):
            changed = list(proofs)
            changed[dead] = proofs[dead][:-8]
            changed[victim] = W.with_words(proofs[victim], [(word, (int(W.words_of(proofs[victim])[word]) + 1) % P)])
            host = host_all(gd, changed, prefixes)
            assert [v for v, _ in host] == [(1, -1, -1) if i == dead else want if i == victim else OK for i in range(B)]
            assert_as_host(prover, gd, changed, prefixes, host)
        # all proofs inactive: nothing is launched, every verdict is the host's
        cut = [b[:-8] for b in proofs]
        assert_as_host(prover, gd, cut, prefixes, host_all(gd, cut, prefixes))
    finally:
        close(gp)


# ---- 4. the first failure wins ------------------------------------------------------------------------------------------------
def test_the_first_failure_wins(prover):
    db, nq = 4, 6
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=nq, pow_bits=0)   # no proof of work: a changed transcript still reaches the queries
    try:
        proofs, prefixes = honest_toy_proofs(prover, gd, db, 3)
        lab = W.layout(*shape)
        w = W.words_of(proofs[1])
        bump = lambda i: (i, (int(w[i]) + 1) % P)
        evals = lambda q: [i for i, l in enumerate(lab) if l[:3] == ("eval", q, 0)]
        cases = {
            # a later round's oracle path and the final polynomial, which every round reads (and the transcript: the indices move)
            "final": [bump(lab.index(("leaf", 4, 0, 0))), bump(lab.index(("final", 0)))],
            # a later round's oracle path and an earlier round's layer: round 1 fails first, by its value or by its path
            "rounds": [bump(lab.index(("leaf", 4, 0, 0))), bump(evals(1)[3])],
            # every value of a round's layer and the same round's oracle path: the path is checked first
            "path first": [bump(i) for i in evals(2)] + [bump(lab.index(("sib", 2, 1, 0)))],
            # every value of a round's layer and that layer's path: the value is checked first
            "value first": [bump(i) for i in evals(2)] + [bump(lab.index(("lsib", 2, 0, 0)))],
        }
        for name, changes in cases.items():
            changed = [proofs[0], W.with_words(proofs[1], changes), proofs[2]]
            host = host_all(gd, changed, prefixes)
            v = host[1][0]
            assert host[0][0] == OK and host[2][0] == OK and v != OK
            if name == "final":
                assert 0 <= v[1] < 4   # a check of an earlier round than the changed leaf's, whichever the moved indices make it
            if name == "rounds":
                assert v in ((8, 1, 0), (9, 1, 0))
            if name == "path first":
                assert v == (7, 2, 1)
            if name == "value first":
                assert v == (8, 2, 0)
            assert_as_host(prover, gd, changed, prefixes, host)
    finally:
        close(gp)


# ---- 5. chunking, and a refused allocation ------------------------------------------------------------------------------------
def mixed_toy_proofs(p, gd, db, B):
    inst = [toy_instance(i, db) for i in range(B)]
    prefixes = [pre for _, pre, _ in inst]
    proofs, _ = gpu_batch(p, gd, [t for t, _, _ in inst], prefixes, [w for _, _, w in inst])
    return proofs, prefixes


def test_chunks_give_identical_verdicts(prover):
    db = 4
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=5)
    try:
        proofs, prefixes = mixed_toy_proofs(prover, gd, db, 5)
        lab = W.layout(*shape)
        i = lab.index(("sib", 3, 2, 5))
        proofs[3] = W.with_words(proofs[3], [(i, (int(W.words_of(proofs[3])[i]) + 1) % P)])   # an honest one, refused on the device
        want = host_all(gd, proofs, prefixes)
        assert [v for v, _ in want] == [OK, (5, -1, 0), (5, -1, 0), (7, 3, 2), (5, -1, 0)]
        for chunk in (1, 2, 0):
            assert_as_host(prover, gd, proofs, prefixes, want, chunk=chunk)
    finally:
        close(gp)


def test_a_refused_device_allocation_is_out_of_memory_and_writes_nothing(prover):
    import cityprover
    db = 4
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=5)   # the description is read on the host: any context's programs do
    try:
        proofs, prefixes = mixed_toy_proofs(prover, gd, db, 3)
        keep_b, ptrs, lens = cityprover._proof_array(proofs)
        B = len(proofs)

        def call(p):
            chs = (cityprover.ChallengerState * B)()
            for i, pre in enumerate(prefixes):
                c = W.challenger(pre)
                ctypes.memmove(ctypes.byref(chs[i]), ctypes.byref(c), ctypes.sizeof(cityprover.ChallengerState))
            before = bytes(chs)
            out = np.full(B, 0x5A5A5A5A, dtype=cityprover.VERDICT)
            rc = p.lib.cp_stark_verify_batch(p.ctx, ctypes.byref(gd), B, None, None, chs, ptrs, lens, 0, cityprover.PATHS_COOP, out.ctypes.data)
            if rc != 0:
                assert bytes(chs) == before and (out == np.full(B, 0x5A5A5A5A, dtype=cityprover.VERDICT)).all(), "a refused call wrote"
                raise cityprover.CityProverError("[%d] %s" % (rc, p.lib.cp_last_error(p.ctx).decode()))
            return out.tobytes(), bytes(chs)

        want = call(prover)
        assert [tuple(int(x) for x in (v["status"], v["query"], v["detail"])) for v in np.frombuffer(want[0], dtype=cityprover.VERDICT)] == \
            [OK, (5, -1, 0), (5, -1, 0)]
        assert walk(call, want) >= 1
    finally:
        close(gp)


# ---- 6. what needs a context to refuse ----------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(prover):
    import cityprover
    db = 4
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=5)
    try:
        proofs, prefixes = honest_toy_proofs(prover, gd, db, 2)
        chs = [W.challenger(pre) for pre in prefixes]
        before = [c.as_tuple() for c in chs]
        with pytest.raises(cityprover.CityProverError, match="path_form"):
            cityprover.stark_verify_batch(prover, gd, chs, proofs, path_form=3)
        bad = W.challenger(prefixes[1])
        bad.n_input = 99
        with pytest.raises(cityprover.CityProverError, match=r"^\[-1\] proof 1"):
            cityprover.stark_verify_batch(prover, gd, [chs[0], bad], proofs)
        assert [c.as_tuple() for c in chs] == before
        lib = cityprover.load_library()
        keep_b, ptrs, lens = cityprover._proof_array(proofs)
        arr = (cityprover.ChallengerState * 2)()
        out = np.full(2, 0x5A5A5A5A, dtype=cityprover.VERDICT)
        assert lib.cp_stark_verify_batch(None, ctypes.byref(gd), 2, None, None, arr, ptrs, lens, 0, 0, out.ctypes.data) == -1   # the context last
        assert b"ctx is NULL" in lib.cp_last_error(None) and (out == np.full(2, 0x5A5A5A5A, dtype=cityprover.VERDICT)).all()
    finally:
        close(gp)


# ---- 7. the existing callers keep their kernel --------------------------------------------------------------------------------
def test_cp_verify_batch_still_launches_one_lane_per_path(prover):
    import cityprover as cp
    import test_gpu_verify_batch as VB
    from test_fri_query_words import DIGEST, SHAPES
    c = SHAPES["db5"]()
    circ = VB.load(prover, c, DIGEST)
    try:
        proof = cp.prove_batch(prover, [circ], [c["public_inputs"]], [c["wires"]])[0]
        for chunk, passes in ((0, 1), (2, 2)):
            got, launches = launches_of(prover, lambda: cp.verify_batch(circ, [proof] * 3, chunk=chunk))
            assert [int(v["status"]) for v in got] == [0, 0, 0]
            assert launches["verify_paths"] == passes and launches["verify_arith"] == passes and "verify_paths_coop" not in launches, dict(launches)
    finally:
        circ.close()


def test_the_forms_launch_the_kernel_they_name(prover):
    db = 4
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=5)
    try:
        proofs, prefixes = honest_toy_proofs(prover, gd, db, 3)
        for form, name, other in ((1, "verify_paths", "verify_paths_coop"), (2, "verify_paths_coop", "verify_paths")):
            (got, _, _), launches = launches_of(prover, lambda: batch(prover, gd, proofs, prefixes, form))
            assert got == [OK] * 3
            assert launches[name] == 1 and launches["verify_arith"] == 1 and other not in launches, dict(launches)
        (got, _, _), launches = launches_of(prover, lambda: batch(prover, gd, proofs, prefixes, 0))
        assert got == [OK] * 3 and launches["verify_paths"] + launches["verify_paths_coop"] == 1
    finally:
        close(gp)
