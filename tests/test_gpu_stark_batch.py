"""cp_stark_prove_batch (include/cityprover.h): B traces of one description in one call. The contract is byte equality, instance by
instance, with cp_stark_prove - held here against the CPU oracle's prover (oracle/stark_air.c, one instance at a time): every
proof and every outgoing challenger, under the host and the device transcript, with and without an extended round and an
injected proof-of-work witness, through every form of the interpreter, across the launch-form thresholds that depend on B, and
after a refused call (a trace element >= p, a refused device allocation). The oracle's proofs are computed once per shape and
instance and shared. The GPU is touched only inside tests."""
import collections
import ctypes
import os

import numpy as np
import pytest

import air_programs as A
import oracle_lib as O
from test_gpu_air import random_map_program
from test_gpu_alloc_faults import clean, walk

pytestmark = pytest.mark.gpu
P = O.P


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    yield p
    O.lib().or_set_threads(1)
    p.close()


def oracle_instance(od, trace, prefix, pow_override, publics=(), globals_=()):
    """(proof bytes, outgoing challenger) of one instance alone"""
    oc = O.challenger_new()
    if len(prefix):
        O.challenger_observe(oc, prefix)
    proof = O.stark_prove(od, trace, oc, publics=publics, globals_=globals_, pow_override=pow_override)
    return proof, O.challenger_tuple(oc)


def gpu_batch(p, gd, traces, prefixes, pows, publics=None, globals_=None):
    """-> (proofs, challenger tuples) of one cp_stark_prove_batch call"""
    import cityprover
    gcs = []
    for pre in prefixes:
        c = cityprover.ChallengerState()
        if len(pre):
            c.observe(pre)
        gcs.append(c)
    got = cityprover.stark_prove_batch(p, gd, traces, gcs, publics=publics, globals_=globals_,
                                       pow_overrides=pows if any(w is not None for w in pows) else None)
    return got, [c.as_tuple() for c in gcs]


def launches_of(p, fn):
    p.profile_begin()
    try:
        out = fn()
    finally:
        prof = p.profile_end()
    return out, collections.Counter({k: v["launches"] for k, v in prof.items() if not k.startswith(("host:", "wait:"))})


# ---- 1. the toy AIR with a lookup ----------------------------------------------------------------------------------------
CHEATS = (None, "value", "fib")
_toy = {}


def toy_instance(i, db):
    """instance i: its trace (honest, a looked-up value outside the table, a broken transition: cycled), its challenger prefix,
    its injected proof-of-work witness (the instances with the looked-up value outside the table have one: an injected witness is
    not a valid one, and the honest instances are verified in full)"""
    return A.lookup_trace(1 << db, cheat=CHEATS[i % 3]), list(range(i + 1, i + 6)), (1000 + i if i % 3 == 1 else None)


def toy_oracle(db, i):
    if (db, i) not in _toy:
        c, ma, mb = A.lookup_programs()
        op = [x.oracle() for x in (c, ma, mb)]
        od, keep = O.stark_desc(db, 1, 2, O.fri_params(db, 1, 2, 5, 12, (2,)), A.LOOKUP_K0, op[0], A.LOOKUP_K1, 3, steps=A.lookup_steps(op[1], op[2]))
        _toy[(db, i)] = oracle_instance(od, *toy_instance(i, db))
    return _toy[(db, i)]


def toy_desc(p, db):
    import cityprover
    gp = [x.gpu(p) for x in A.lookup_programs()]
    gd, keep = cityprover.stark_desc(db, 1, 2, cityprover.fri_params(db, 1, 2, 5, 12, (2,)), A.LOOKUP_K0, gp[0], A.LOOKUP_K1, 3,
                                     steps=A.lookup_steps(gp[1], gp[2]))
    return gd, keep, gp


def toy_batch_matches(p, gd, db, B):
    inst = [toy_instance(i, db) for i in range(B)]
    (got, chs), launches = launches_of(p, lambda: gpu_batch(p, gd, [t for t, _, _ in inst], [pre for _, pre, _ in inst], [w for _, _, w in inst]))
    assert len(got) == B
    for i in range(B):
        want, want_ch = toy_oracle(db, i)
        assert got[i] == want, (db, B, i)
        assert chs[i] == want_ch, (db, B, i)
    return got, launches


@pytest.mark.parametrize("device_transcript", [0, 1])
@pytest.mark.parametrize("db", [4, 7])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_toy_air_batch_equals_the_oracle_instance_by_instance(prover, db, B, device_transcript):
    import cityprover
    gd, keep, gp = toy_desc(prover, db)
    prover.set_device_transcript(device_transcript)
    try:
        got, launches = toy_batch_matches(prover, gd, db, B)
        # B instances share every launch of the STARK's own steps: two map steps, one inversion, one prefix sum, one quotient
        assert {k: launches[k] for k in ("air_map", "cubic_batch_inverse", "column_prefix_sum", "air_quotient", "air_finish")} == \
            {"air_map": 2, "cubic_batch_inverse": 1, "column_prefix_sum": 1, "air_quotient": 1, "air_finish": 1}, dict(launches)
        for i in range(B):
            v = cityprover.ChallengerState()
            v.observe(toy_instance(i, db)[1])
            if CHEATS[i % 3] is None:
                cityprover.stark_verify(gd, v, got[i])
                assert v.as_tuple() == toy_oracle(db, i)[1]
            else:
                with pytest.raises(cityprover.CityProverError, match="quotient identity fails at zeta"):
                    cityprover.stark_verify(gd, v, got[i])
    finally:
        prover.set_device_transcript(-1)
        for g in gp:
            g.close()


LOCKSTEP_PREFIXES = (0, 1, 3, 7, 8, 9, 13)


@pytest.mark.parametrize("device_transcript", [0, 1])
def test_prefixes_of_every_buffer_state_in_one_batch(prover, device_transcript):
    """transcript.h `k_step` reads the buffer counters of a wave's first challenger for all five. Seven instances (two waves, the
    second partial) whose incoming challengers have absorbed 0, 1, 3, 7, 8, 9 and 13 elements — every one in another buffer
    state: empty, partly filled, one short of a permutation, just permuted, permuted and filling again — must still prove what the
    oracle proves one at a time, and hand back its challenger."""
    db, B = 4, len(LOCKSTEP_PREFIXES)
    c, ma, mb = A.lookup_programs()
    op = [x.oracle() for x in (c, ma, mb)]
    od, okeep = O.stark_desc(db, 1, 2, O.fri_params(db, 1, 2, 5, 12, (2,)), A.LOOKUP_K0, op[0], A.LOOKUP_K1, 3, steps=A.lookup_steps(op[1], op[2]))
    rng = np.random.default_rng(41)
    traces = [A.lookup_trace(1 << db, cheat=CHEATS[i % 3]) for i in range(B)]
    prefixes = [rng.integers(0, P, n, dtype=np.uint64) for n in LOCKSTEP_PREFIXES]
    pows = [None] * B
    gd, keep, gp = toy_desc(prover, db)
    prover.set_device_transcript(device_transcript)
    try:
        batch_matches(prover, gd, od, traces, prefixes, pows)
    finally:
        prover.set_device_transcript(-1)
        for g in gp:
            g.close()


# ---- 2. per-instance uniforms on the seeded small random shapes----------------------------------------------------------
def random_shape(seed):
    """the shape generator of test_gpu_air.py::test_stark_prove_bytes_on_small_random_shapes (same seeds, same draws), as builders"""
    rng = np.random.default_rng(9000 + seed)
    db = int(rng.integers(3, 9))
    rb = int(rng.integers(1, 4))
    q = int(rng.integers(1, min(rb, 2) + 1))
    na = int(rng.integers(1, 5))
    k0 = int(rng.integers(1, 12))
    k1 = 0 if seed % 3 == 0 else 3 * int(rng.integers(1, 4))
    n_pub, n_glob = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    n_rch = int(rng.integers(1, 4)) if k1 else 0
    ch = int(rng.integers(0, min(db + rb, 4) + 1))
    cons = A.random_program(seed + 50, k0 + k1, int(rng.integers(30, 400)), n_public=n_pub, n_global=n_glob, n_challenge=n_rch, max_degree=(1 << q) + 1)
    steps = []
    if k1:
        kinds = ["map"] + [("cubic_inverse", "prefix_sum", "map")[int(x)] for x in rng.integers(0, 3, int(rng.integers(0, 3)))]
        for kind in kinds:
            if kind == "map":
                steps.append(("map", random_map_program(rng, k0, k1, n_pub, n_glob, n_rch, set(int(x) for x in rng.integers(0, k1, 2)))))
            elif kind == "cubic_inverse":
                cnt = int(rng.integers(1, k1 // 3 + 1))
                first = 3 * int(rng.integers(0, k1 // 3 - cnt + 1))
                steps.append(("cubic_inverse", first, cnt, A.CUBIC_MODULUS if rng.random() < 0.5 else (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))))
            else:
                cnt = int(rng.integers(1, k1 + 1))
                steps.append(("prefix_sum", int(rng.integers(0, k1 - cnt + 1)), cnt, bool(rng.integers(0, 2))))
    arity = ()
    d = db
    while d > 3 and d + rb - 2 >= ch and rng.random() < 0.7 and len(arity) < 3:
        a = int(rng.integers(1, 3))
        if d - a < 1 or d - a + rb < ch:
            break
        arity += (a,)
        d -= a
    pow_bits, nq = int(rng.integers(0, 9)), int(rng.integers(1, 12))
    return dict(db=db, rb=rb, q=q, na=na, k0=k0, k1=k1, n_pub=n_pub, n_glob=n_glob, n_rch=n_rch, ch=ch, cons=cons, steps=steps, arity=arity,
                pow_bits=pow_bits, nq=nq, rng=rng)


def descs_of(p, s):
    """(gpu desc, oracle desc, keep-alives, gpu programs to close) of a shape dict (cons, steps with builders)"""
    import cityprover
    progs = [s["cons"].gpu(p)]
    sg, so = [], []
    for st in s["steps"]:
        if st[0] == "map":
            progs.append(st[1].gpu(p))
            sg.append(("map", progs[-1]))
            so.append(("map", st[1].oracle()))
        else:
            sg.append(st)
            so.append(st)
    fri = (s["db"], s["rb"], s["ch"], s["pow_bits"], s["nq"], s["arity"])
    gd, gk = cityprover.stark_desc(s["db"], s["q"], s["na"], cityprover.fri_params(*fri), s["k0"], progs[0], s["k1"], s["n_rch"], n_public=s["n_pub"],
                                   n_global=s["n_glob"], steps=sg)
    od, ok = O.stark_desc(s["db"], s["q"], s["na"], O.fri_params(*fri), s["k0"], s["cons"].oracle(), s["k1"], s["n_rch"], n_public=s["n_pub"],
                          n_global=s["n_glob"], steps=so)
    return gd, od, (gk, ok), progs


def batch_matches(p, gd, od, traces, prefixes, pows, pubs=None, globs=None):
    B = len(traces)
    got, chs = gpu_batch(p, gd, traces, prefixes, pows, publics=pubs, globals_=globs)
    assert len(got) == B
    for i in range(B):
        want, want_ch = oracle_instance(od, traces[i], prefixes[i], pows[i], () if pubs is None else pubs[i], () if globs is None else globs[i])
        assert got[i] == want, i
        assert chs[i] == want_ch, i


@pytest.mark.parametrize("seed", range(10))
def test_small_random_shapes_with_per_instance_publics_globals_and_challenges(prover, seed):
    """every instance has its own trace, publics, globals and transcript prefix (so its own round challenges and alphas): a wrong
    instance stride in the uniform, alpha or weight tables, or in a column pointer table, shows here"""
    B = 3
    s = random_shape(seed)
    rng = s["rng"]
    gd, od, keep, progs = descs_of(prover, s)
    traces = [rng.integers(0, P, (s["k0"], 1 << s["db"]), dtype=np.uint64) for _ in range(B)]
    pubs = rng.integers(0, P, (B, s["n_pub"]), dtype=np.uint64) if s["n_pub"] else None
    globs = rng.integers(0, P, (B, s["n_glob"]), dtype=np.uint64) if s["n_glob"] else None
    prefixes = [rng.integers(0, P, int(rng.integers(0, 11)), dtype=np.uint64) for _ in range(B)]
    prover.set_device_transcript(seed % 2)
    try:
        batch_matches(prover, gd, od, traces, prefixes, [None, 12345, None], pubs, globs)
    finally:
        prover.set_device_transcript(-1)
        for g in progs:
            g.close()


# ---- 3. the forms of the interpreter ---------------------------------------------------------------------------------------
# 2^6 rows: the case the forms are asked at (a launch that small keeps one point per lane whatever is asked for); 2^11 rows x 4
# quotient points x 3 instances = 24576 points: the least at which three instances together keep four points per lane
FORM_SHAPES = {6: dict(db=6, rb=2, q=1, ch=1, arity=(2,)), 11: dict(db=11, rb=2, q=2, ch=2, arity=(2, 2))}
_forms = {}


def form_case(db):
    """a tangled constraint program (operands from anywhere in the program: long-lived temporaries) over 6 + 3 columns, the
    extended columns by a map step with an inversion; three instances with their own trace, public, global and prefix"""
    if db not in _forms:
        f = FORM_SHAPES[db]
        k0, k1 = 6, 3
        cons = A.random_program(9300 + db, k0 + k1, 600, n_public=1, n_global=1, n_challenge=1, max_degree=(1 << f["q"]) + 1, far=0.5)
        m = A.Builder(A.MAP, k0 + k1, n_public=1, n_global=1, n_challenge=1, n_out_columns=k1)
        for j in range(k1):
            m.store(j, m.inv(m.add(m.mul(m.local(j), m.challenge(0)), m.sub(m.next((j + 1) % k0), m.public(0)))))
        s = dict(f, na=2, k0=k0, k1=k1, n_pub=1, n_glob=1, n_rch=1, cons=cons, steps=[("map", m), ("prefix_sum", 0, 2, False)], pow_bits=4, nq=5)
        rng = np.random.default_rng(9400 + db)
        traces = [rng.integers(0, P, (k0, 1 << db), dtype=np.uint64) for _ in range(3)]
        pubs, globs = rng.integers(0, P, (3, 1), dtype=np.uint64), rng.integers(0, P, (3, 1), dtype=np.uint64)
        prefixes, pows = [[i + 1, 7] for i in range(3)], [None, 99, None]
        fri = (s["db"], s["rb"], s["ch"], s["pow_bits"], s["nq"], s["arity"])
        od, ok = O.stark_desc(s["db"], s["q"], s["na"], O.fri_params(*fri), k0, cons.oracle(), k1, 1, n_public=1, n_global=1,
                              steps=[("map", m.oracle()), s["steps"][1]])
        want = [oracle_instance(od, traces[i], prefixes[i], pows[i], pubs[i], globs[i]) for i in range(3)]
        _forms[db] = (s, traces, pubs, globs, prefixes, pows, want)
    return _forms[db]


@pytest.mark.parametrize("db,options", [(6, dict(AIR_POINTS_PER_LANE=1)), (6, dict(AIR_POINTS_PER_LANE=2)), (6, dict(AIR_POINTS_PER_LANE=4)),
                                        (6, dict(AIR_LDS_SLOTS=2)), (6, dict(AIR_TARGET_WAVES=1 << 30)),
                                        (11, dict(AIR_POINTS_PER_LANE=2)), (11, dict(AIR_POINTS_PER_LANE=4)),
                                        (11, dict(AIR_POINTS_PER_LANE=4, AIR_LDS_SLOTS=2, AIR_TARGET_WAVES=1 << 30))])
def test_interpreter_forms_give_the_same_bytes(db, options):
    """points per lane, slots spilled to the global scratch array (two slots in LDS, the rest of a tangled program's in the
    array: the spill index carries the instance), more than one segment: the bytes are the oracle's under every setting"""
    import cityprover
    s, traces, pubs, globs, prefixes, pows, want = form_case(db)
    p = cityprover.Prover(0)
    try:
        for k, v in options.items():
            p.set_option(k, v)
        gd, od, keep, progs = descs_of(p, s)
        try:
            info = progs[0].info()
            assert info["n_slots"] > 2 and info["n_segments_max"] > 1   # slots do spill at two LDS slots; the program can be cut
            got, chs = gpu_batch(p, gd, traces, prefixes, pows, publics=pubs, globals_=globs)
            for i in range(3):
                assert got[i] == want[i][0], (db, options, i)
                assert chs[i] == want[i][1], (db, options, i)
        finally:
            for g in progs:
                g.close()
    finally:
        p.close()


# ---- 4. launch-form thresholds that depend on B ---------------------------------------------------------------------------
def test_toy_air_at_2_10_rows_five_instances(prover):
    """2^10 rows, rate 2: 2048 leaves x 5 trees cross the thresholds below which the leaf hashes take the cooperative form"""
    gd, keep, gp = toy_desc(prover, 10)
    try:
        toy_batch_matches(prover, gd, 10, 5)
    finally:
        for g in gp:
            g.close()


def test_sha256_stark_width_two_instances(prover):
    """the shape of test_gpu_air.py::test_stark_prove_bytes_at_the_sha256_stark_width (418 + 912 columns, 2^10 rows, a 10^4-op
    constraint program, a 912-store map, 304 cubic inversions, prefix sums of all 912 columns, 84 queries, arity 16), two
    instances: the split combine of FRI, the map segments and the inversions across instances"""
    import cityprover
    db, k0, k1 = 10, 418, 912
    cons = A.gadget_program(77, k0 + k1, 10500, n_public=4, n_global=0, n_challenge=6, max_degree=3)
    m = A.Builder(A.MAP, k0 + k1, n_public=4, n_challenge=6, n_out_columns=k1)
    ch = [m.challenge(i) for i in range(6)]
    for j in range(k1):
        v = m.add(m.mul(m.local(j % k0), ch[j % 6]), m.next((7 * j + 1) % k0))
        m.store(j, m.sub(v, m.public(j % 4)) if j % 3 else v)
    s = dict(db=db, rb=1, q=1, na=2, k0=k0, k1=k1, n_pub=4, n_glob=0, n_rch=6, ch=4, cons=cons, arity=(4,), pow_bits=16, nq=84,
             steps=[("map", m), ("cubic_inverse", 0, 304, A.CUBIC_MODULUS), ("prefix_sum", 0, k1, False)])
    gd, od, keep, progs = descs_of(prover, s)
    rng = np.random.default_rng(8)
    traces = [rng.integers(0, P, (k0, 1 << db), dtype=np.uint64) for _ in range(2)]
    pubs = rng.integers(0, P, (2, 4), dtype=np.uint64)
    try:
        batch_matches(prover, gd, od, traces, [[], [3]], [None, None], pubs)
    finally:
        for g in progs:
            g.close()


# ---- 5. failure semantics ---------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing_and_the_context_goes_on(prover):
    import cityprover
    db, B = 4, 3
    gd, keep, gp = toy_desc(prover, db)
    lib = prover.lib
    try:
        traces = [np.array(toy_instance(i, db)[0], dtype=np.uint64, copy=True) for i in range(B)]
        traces[1][A.LOOKUP_K0 - 1, 5] = P + 5
        tp = (ctypes.c_void_p * B)(*[t.ctypes.data for t in traces])
        chs = (cityprover.ChallengerState * B)()
        for i in range(B):
            c = cityprover.ChallengerState().observe(toy_instance(i, db)[1])
            ctypes.memmove(ctypes.byref(chs[i]), ctypes.byref(c), ctypes.sizeof(c))
        before = bytes(chs)
        outs, lens = (ctypes.POINTER(ctypes.c_uint8) * B)(), (ctypes.c_size_t * B)()
        sentinel = 0x5A5A5A50
        for i in range(B):
            outs[i], lens[i] = ctypes.cast(sentinel, ctypes.POINTER(ctypes.c_uint8)), 7

        def untouched():
            return bytes(chs) == before and all(ctypes.cast(outs[i], ctypes.c_void_p).value == sentinel and lens[i] == 7 for i in range(B))
        rc = lib.cp_stark_prove_batch(prover.ctx, ctypes.byref(gd), B, tp, 0, None, None, chs, None, None, outs, lens)
        msg = lib.cp_last_error(prover.ctx).decode()
        assert rc == -1 and "instance 1" in msg and "not canonical" in msg, (rc, msg)
        assert untouched()
        # refusals that need a context: an instance's trace pointer, challenger, proof-of-work witness (each names the instance)
        tp_null = (ctypes.c_void_p * B)(traces[0].ctypes.data, traces[0].ctypes.data, None)
        assert lib.cp_stark_prove_batch(prover.ctx, ctypes.byref(gd), B, tp_null, 0, None, None, chs, None, None, outs, lens) == -1
        assert "instance 2" in lib.cp_last_error(prover.ctx).decode()
        up, ov = (ctypes.c_int * B)(0, 1, 0), (ctypes.c_uint64 * B)(0, P, 0)
        assert lib.cp_stark_prove_batch(prover.ctx, ctypes.byref(gd), B, tp, 0, None, None, chs, up, ov, outs, lens) == -1
        assert "instance 1" in lib.cp_last_error(prover.ctx).decode() and "pow witness" in lib.cp_last_error(prover.ctx).decode()
        chs[2].n_input = 9
        before_bad = bytes(chs)
        assert lib.cp_stark_prove_batch(prover.ctx, ctypes.byref(gd), B, tp, 0, None, None, chs, None, None, outs, lens) == -1
        assert "instance 2" in lib.cp_last_error(prover.ctx).decode() and bytes(chs) == before_bad
        assert lib.cp_stark_prove_batch(prover.ctx, None, B, tp, 0, None, None, chs, None, None, outs, lens) == -1
        chs[2].n_input = 5
        assert untouched()
        # the same call with good traces: the oracle's bytes (the flag of the device scan does not stick)
        toy_batch_matches(prover, gd, db, B)
    finally:
        for g in gp:
            g.close()


# ---- 6. a refused device allocation anywhere inside the call ----------------------------------------------------------------
def test_every_allocation_of_a_batch_call_may_be_refused():
    import cityprover
    db, B = 4, 2
    inst = [toy_instance(i, db) for i in range(B)]

    def call(p):
        gd, keep, gp = toy_desc(p, db)
        try:
            got, chs = gpu_batch(p, gd, [t for t, _, _ in inst], [pre for _, pre, _ in inst], [w for _, _, w in inst])
            return list(zip(got, chs))
        finally:
            for g in gp:
                g.close()
    want = clean(call)
    assert want == [toy_oracle(db, i) for i in range(B)]
    assert walk(call, want) >= 6   # the value columns, the compiled programs, the selector table, the arena, the pinned area
