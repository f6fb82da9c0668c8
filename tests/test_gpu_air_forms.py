"""Every launch form of the AIR interpreter (air.h k_run<MODE, K>, stark.inc air_run) pinned to the CPU oracle (oracle/stark_air.c).

The forms: 1, 2 or 4 points per lane (CITYPROVER_AIR_POINTS_PER_LANE; a launch too small for K falls back to fewer), how many
per-lane temporaries stay in LDS (CITYPROVER_AIR_LDS_SLOTS: none spilled, some, all but one), and how finely the program is cut
into segments (CITYPROVER_AIR_TARGET_WAVES: one segment, the default, as many as the roots allow up to 1024). At four points per
lane a program of more than 80 temporaries needs more LDS than a gfx950 workgroup may have: air_run clamps the LDS slots to what
the device grants and spills the rest. Column prefetch (CITYPROVER_AIR_PREFETCH, cached per process) runs in a child process.
Each case asserts the interpreter launch it expects from the profile. The GPU is touched only inside tests."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import air_programs as A
import oracle_lib as O
from air_programs import quotient_case

pytestmark = pytest.mark.gpu
P = O.P
WAVE = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POINTS = (1, 2, 4)
SLOTS = (1, 10, 120)
WAVES = (1, 8192, 1 << 30)

# switch -> the tests of this module that set it (tests/test_switch_coverage.py)
FORMS = {
    "AIR_POINTS_PER_LANE": ["test_quotient_matrix_small_programs", "test_quotient_matrix_wide_program", "test_stark_prove_bytes_at_one_and_four_points"],
    "AIR_LDS_SLOTS": ["test_quotient_matrix_small_programs", "test_quotient_matrix_wide_program", "test_map_programs_under_slot_and_wave_rows"],
    "AIR_TARGET_WAVES": ["test_quotient_matrix_small_programs", "test_quotient_matrix_wide_program", "test_map_programs_under_slot_and_wave_rows"],
}


def points_per_lane(M, want):
    """stark.inc cp_air_quotient_commit: K halves until the launch gives every SIMD a few waves' worth of points"""
    K = 4 if want >= 4 else 2 if want >= 2 else 1
    while K > 1 and M < WAVE * K * 64:
        K >>= 1
    return K


def forced(**opts):
    import cityprover
    p = cityprover.Prover(0)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def measured(prover, fn):
    prover.profile_begin()
    try:
        out = fn()
    finally:
        prof = prover.profile_end()
    return out, collections.Counter({k: v["launches"] for k, v in prof.items() if k in ("air_quotient", "air_map")})


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    yield
    O.lib().or_set_threads(1)


ROWS = [(k, s, w) for k in POINTS for s in SLOTS for w in WAVES]


def small_cases():
    """three seeded small programs, 4-256 rows (partial waves and tails)"""
    out = []
    for seed, db in ((1, 2), (2, 5), (3, 8)):
        rng = np.random.default_rng(7000 + seed)
        rb = 2
        q = int(rng.integers(1, rb + 1))
        ks = [int(rng.integers(1, 9)) for _ in range(2)]
        b = A.random_program(7100 + seed, sum(ks), int(rng.integers(100, 600)), n_public=1, n_global=1, n_challenge=2, max_degree=(1 << q) + 1)
        out.append((b, ks, db, rb, q, int(rng.integers(1, 4)), 1, seed))
    return out


@pytest.mark.parametrize("k,slots,waves", ROWS)
def test_quotient_matrix_small_programs(k, slots, waves):
    p = forced(AIR_POINTS_PER_LANE=k, AIR_LDS_SLOTS=slots, AIR_TARGET_WAVES=waves)
    try:
        for b, ks, db, rb, q, na, ch, seed in small_cases():
            _, launches = measured(p, lambda: quotient_case(p, b, ks, db, rb, q, na, ch, seed))
            assert launches == {"air_quotient": 1}, (k, slots, waves, db)
    finally:
        p.close()


# the wide program: more than 80 live temporaries (120 LDS slots at four points per lane would ask for 240 KiB of LDS), at
# 2^13 rows x 2 (quotient degree bits 1): 16384 points, the least that keeps four points per lane
WIDE_DB, WIDE_RB, WIDE_Q, WIDE_KS = 13, 1, 1, [24, 16]
_wide = {}


def wide_case():
    if "case" not in _wide:
        b = A.random_program(8101, sum(WIDE_KS), 2500, n_public=1, n_global=1, n_challenge=2, max_degree=3, far=0.5)
        rng = np.random.default_rng(8102)
        n = 1 << WIDE_DB
        traces = [rng.integers(0, P, (k, n), dtype=np.uint64) for k in WIDE_KS]
        pub, glo, cha = (rng.integers(0, P, k, dtype=np.uint64) for k in (1, 1, 2))
        alphas = rng.integers(0, P, 2, dtype=np.uint64)
        Ob = [O.Batch(t, WIDE_RB, 2) for t in traces]
        try:
            want = O.air_quotient(b.oracle(), Ob, WIDE_Q, alphas, pub, glo, cha)
        finally:
            for x in Ob:
                x.close()
        oq = O.Batch(want, WIDE_RB, 2, True)
        _wide["case"] = (b, traces, pub, glo, cha, alphas, want, oq.cap())
        oq.close()
    return _wide["case"]


@pytest.mark.parametrize("k,slots,waves", ROWS)
def test_quotient_matrix_wide_program(k, slots, waves):
    import cityprover
    b, traces, pub, glo, cha, alphas, want, want_cap = wide_case()
    assert points_per_lane(len(traces[0][0]) << WIDE_Q, k) == k      # the shape keeps the form that was asked for
    p = forced(AIR_POINTS_PER_LANE=k, AIR_LDS_SLOTS=slots, AIR_TARGET_WAVES=waves)
    G = [cityprover.PolyBatch(p, t, WIDE_RB, 2) for t in traces]
    g = b.gpu(p)
    try:
        assert g.info()["n_slots"] > 80          # what makes the LDS budget bind at four points per lane
        Q, launches = measured(p, lambda: cityprover.air_quotient_commit(p, g, G, WIDE_Q, alphas, pub, glo, cha))
        try:
            assert (Q.coeffs() == want).all(), (k, slots, waves)
            assert (Q.cap() == want_cap).all()
        finally:
            Q.close()
        assert launches == {"air_quotient": 1}
    finally:
        g.close()
        for x in G:
            x.close()
        p.close()


def next_row_inv_program():
    """test_gpu_air.py test_map_programs_match_oracle: next-row loads wrap around, INV maps 0 to 0, unstored columns stay"""
    b = A.Builder(A.MAP, 2, n_public=1, n_out_columns=3)
    b.store(0, b.add(b.next(0), b.public(0)))
    b.store(2, b.inv(b.sub(b.local(1), b.local(0))))
    return b


@pytest.mark.parametrize("slots,waves", [(s, w) for s in SLOTS for w in WAVES])
def test_map_programs_under_slot_and_wave_rows(slots, waves):
    import cityprover
    _, ma, mb = A.lookup_programs()
    rng = np.random.default_rng(40 + slots + waves % 97)
    beta = rng.integers(0, P, 3, dtype=np.uint64)
    p = forced(AIR_LDS_SLOTS=slots, AIR_TARGET_WAVES=waves)
    try:
        for n in (1, 65, 1000, 1 << 12):
            cols = rng.integers(0, P, (22, n), dtype=np.uint64)
            for b in (ma, mb):
                g, o = b.gpu(p), b.oracle()
                try:
                    got, launches = measured(p, lambda: cityprover.air_map(p, g, cols, challenges=beta))
                    assert (got == o.map(cols, challenges=beta)).all(), (slots, waves, n)
                    assert launches == {"air_map": 1}
                finally:
                    g.close()
        b = next_row_inv_program()
        cols = rng.integers(0, P, (2, 300), dtype=np.uint64)
        cols[1, 17] = cols[0, 17]
        g, o = b.gpu(p), b.oracle()
        try:
            got, launches = measured(p, lambda: cityprover.air_map(p, g, cols, publics=[5]))
        finally:
            g.close()
        assert (got == o.map(cols, publics=[5])).all() and got[2, 17] == 0 and (got[1] == 0).all()
        assert launches == {"air_map": 1}
    finally:
        p.close()


@pytest.mark.parametrize("k", [1, 4])
def test_stark_prove_bytes_at_one_and_four_points(k):
    """the whole prover (commit, extended round with a map step, quotient, FRI) == the oracle's, 2^12 rows x 4 quotient points"""
    import cityprover
    db, rb, q, na, ch, k0, k1, n_rch = 12, 2, 2, 2, 2, 6, 3, 1
    assert points_per_lane(1 << (db + q), k) == k
    rng = np.random.default_rng(9100)
    cons = A.random_program(9150, k0 + k1, 300, n_public=1, n_global=0, n_challenge=n_rch, max_degree=(1 << q) + 1)
    m = A.Builder(A.MAP, k0 + k1, n_public=1, n_challenge=n_rch, n_out_columns=k1)
    for j in range(k1):
        m.store(j, m.inv(m.add(m.mul(m.local(j), m.challenge(0)), m.next((j + 1) % k0))))
    p = forced(AIR_POINTS_PER_LANE=k)
    gcons, gm = cons.gpu(p), m.gpu(p)
    try:
        fri = (db, rb, ch, 4, 6, (2, 2))
        gd, gk = cityprover.stark_desc(db, q, na, cityprover.fri_params(*fri), k0, gcons, k1, n_rch, n_public=1, steps=[("map", gm)])
        od, ok = O.stark_desc(db, q, na, O.fri_params(*fri), k0, cons.oracle(), k1, n_rch, n_public=1, steps=[("map", m.oracle())])
        trace = rng.integers(0, P, (k0, 1 << db), dtype=np.uint64)
        pub = rng.integers(0, P, 1, dtype=np.uint64)
        oc, gc = O.challenger_new(), cityprover.ChallengerState()
        want = O.stark_prove(od, trace, oc, publics=pub)
        got, launches = measured(p, lambda: cityprover.stark_prove(p, gd, trace, gc, publics=pub))
        assert got == want
        assert gc.as_tuple() == O.challenger_tuple(oc)
        assert launches["air_quotient"] == 1 and launches["air_map"] == 1, dict(launches)
    finally:
        gcons.close()
        gm.close()
        p.close()


CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import numpy as np
import cityprover
import air_programs as A
import oracle_lib as O
from air_programs import quotient_case
p = cityprover.Prover(0)
b = A.random_program(7301, 9, 400, n_public=1, n_global=1, n_challenge=2, max_degree=3)
quotient_case(p, b, [5, 4], 7, 2, 1, 2, 1, 7301)
_, ma, _ = A.lookup_programs()
rng = np.random.default_rng(7302)
cols = rng.integers(0, O.P, (22, 1000), dtype=np.uint64)
beta = rng.integers(0, O.P, 3, dtype=np.uint64)
g = ma.gpu(p)
assert (cityprover.air_map(p, g, cols, challenges=beta) == ma.oracle().map(cols, challenges=beta)).all()
g.close()
p.close()
print("prefetch ok")
"""


def test_prefetch_in_a_child_process():
    """CITYPROVER_AIR_PREFETCH is read once per process (a function-static): one quotient case and one map case in a fresh child"""
    env = dict(os.environ, CITYPROVER_AIR_PREFETCH="1")
    code = CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "city-rollup_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0 and "prefetch ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
