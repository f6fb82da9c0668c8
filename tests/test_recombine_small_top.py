"""The recombination with a small top word (poseidon.h `recombine_s`, `repair_s`, gl.h `fold_top_open` / `fold_repair`) and the partial
rounds with the b block in its triangular basis (`dom_mul2_b`, `dom_next_z_b`), instantiated on the host (tests/recombine_sim): against
exact integers, against the tables gen_tables.py derives, against the dense forms, `permute_textbook` and the oracle. CPU only."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
import arith_cases as AC
import recombine_cases as RC
from recombine_cases import EPS, P, TABLES, p64, pd

PERMUTE, ABSORB, SQUEEZE, NODE, TEXTBOOK = range(5)
LIVE = {PERMUTE: (slice(0, 12), True), ABSORB: (slice(8, 12), False), SQUEEZE: (slice(0, 4), True), NODE: (slice(0, 4), True)}
TOP_MAX = 1 << 20


@pytest.fixture(scope="module")
def hs():
    lib = RC.host_lib("host")
    assert lib.rs_flags() == 7, "the default build: small top word, triangular b block, planes in units of 2^32"
    return lib


@pytest.fixture(scope="module")
def hs_v1():
    lib = RC.host_lib("host_v1")
    assert lib.rs_flags() == 4, "the A/B build: recombine_d and the dense b block"
    return lib


@pytest.fixture(scope="module")
def consts():
    return RC.wanted_constants()


def recombine(hs, table, i, l, h):
    w = ctypes.c_int(-1)
    r = hs.rs_recombine(table, i, RC.as_arg(table, l), RC.as_arg(table, h), ctypes.byref(w))
    return r, w.value


# ---- the tables -----------------------------------------------------------------------------------------------------------------
def test_tables_decode_to_the_constants_of_gen_tables(hs, consts):
    """every entry: the mantissas of its two doubles are the halves of c - B (1 + 2^32) + T0 (2^32 - 1), T0 the literal of its family"""
    import gen_tables as G
    lits = G.top0_literals()
    assert lits == {"FULL": 0x43380000, "PARTIAL": 0x43380000 - (1 << 19), "PARTIAL32": 0x41380000 - (1 << 19)}
    for table, (name, lit, B, _) in TABLES.items():
        assert RC.parse_literal(lit) == lits[lit] == hs.rs_top0(table)
        want = consts[table]
        assert len(RC.parse_table(name)) == 2 * len(want)
        for i, c in enumerate(want):
            c0, c1 = RC.halves(table, i)
            assert 0 <= c0 < 1 << 32 and 0 <= c1 < 1 << 32
            assert (c0 + (c1 << 32) + B * (1 + (1 << 32)) - lits[lit] * (1 << 64)) % P == c, (name, i)
    # the margins are the ones the bounds of the limbs give
    assert G.top0_margin(G.FULL_LIMBS) == 0 and G.top0_margin(G.PARTIAL_LIMBS) == 1 << 19


# ---- the recombination against exact integers -----------------------------------------------------------------------------------
def test_recombine_on_the_limb_pairs_of_recombine_d(hs, consts):
    for table in (1, 2, 3, 4):
        for i in (0, len(consts[table]) - 1, 5):
            for l, h in AC.recombine_limbs():
                r, w = recombine(hs, table, i, l, h)
                assert r % P == (l + (h << 32) + consts[table][i]) % P, (table, i, l, h)
                top, lo = RC.top_of(table, i, l, h)
                assert 0 <= top <= TOP_MAX and w == (lo + top * EPS >= 1 << 64)
                assert hs.rs_top(table, i, RC.as_arg(table, l), RC.as_arg(table, h)) == top
    # a full-round layer: non-negative limbs up to 264 (2^32 - 1)
    rng = np.random.default_rng(5)
    hi = 264 * EPS
    for i in (0, 17, 359, 360):
        for l, h in [(0, 0), (hi, hi), (0, hi), (hi, 0), (1, 1)] + [tuple(int(v) for v in rng.integers(0, hi, 2)) for _ in range(40)]:
            r, w = recombine(hs, 0, i, l, h)
            assert r % P == (l + (h << 32) + consts[0][i]) % P
            top, _ = RC.top_of(0, i, l, h)
            assert 0 <= top <= 266


def test_top_word_at_the_proven_bounds(hs, consts):
    """the top word stays in [0, 2^20] at the ends of the range of the limbs, both signs of l and h, whatever the constant"""
    import gen_tables as G
    lo, hi = G.PARTIAL_LIMBS
    seen = set()
    for table in (1, 2, 3, 4):
        for i in range(len(consts[table])):
            for l in (lo, hi, -1, 0, 1):
                for h in (lo, lo + 1, hi, hi - 1, -1, 0):
                    top = hs.rs_top(table, i, RC.as_arg(table, l), RC.as_arg(table, h))
                    assert top == RC.top_of(table, i, l, h)[0] and 0 <= top <= TOP_MAX, (table, i, l, h, top)
                    seen.add(top)
                    if abs(l) <= AC.RECOMBINE_LIM and abs(h) <= AC.RECOMBINE_LIM:
                        assert recombine(hs, table, i, l, h)[0] % P == (l + (h << 32) + consts[table][i]) % P
    assert min(seen) == 0 and max(seen) >= TOP_MAX - 1, "the bounds were not reached"
    lo, hi = G.FULL_LIMBS
    for i in range(361):
        for h in (lo, hi):
            assert 0 <= hs.rs_top(0, i, float(hi), float(h)) <= 266


def test_constructed_wraps_in_both_units(hs, consts):
    """limb pairs whose middle word is within the top word of 2^32: the fold wraps, the repair restores the value; a middle word
    just below does not wrap"""
    wraps = 0
    for table in (0, 1, 2, 3, 4):
        ks = (2, 200) if table == 0 else (-(1 << 18), -3, 0, 7, 1 << 18)
        ls = (0, 5, 1 << 40) if table == 0 else (0, -1, 123456789012345, -(1 << 50), 1 << 50)
        for i in (0, 3, len(consts[table]) - 1):
            for l in ls:
                for k in ks:
                    for want in (True, False):
                        h = RC.wrap_pair(table, i, l, k, wraps=want)
                        r, w = recombine(hs, table, i, l, h)
                        assert w == want, (table, i, l, k)
                        assert r % P == (l + (h << 32) + consts[table][i]) % P, (table, i, l, k)
                        wraps += w
    assert wraps >= 150


def test_sites_equal_single_recombinations(hs, consts):
    """the three sites as the permutation runs them (groups of recombinations behind one test) give what single recombinations give,
    with the wrap in every position of the twelve, and count one run of the rare path per group that wraps"""
    runs = (ctypes.c_ulonglong * 3)()
    hs.rs_wrap_runs(runs, 1)
    for site, table, idx in ((0, 0, 3), (0, 0, 30), (2, 4, 0)):
        n = 14
        l = np.zeros((n, 12))
        h = np.zeros((n, 12))
        want = np.zeros((n, 12), np.uint64)
        for e in range(n):                       # element e < 12: the wrap in position e; 12: nowhere; 13: everywhere
            for k in range(12):
                i = (idx * 12 + k if idx < 30 else 360) if table == 0 else k
                li = 1000 * e + k
                hi_ = RC.wrap_pair(table, i, li, 5, wraps=(e == k or e == 13))
                l[e, k], h[e, k] = RC.as_arg(table, li), RC.as_arg(table, hi_)
                want[e, k] = recombine(hs, table, i, li, hi_)[0]
        out = np.zeros((n, 12), np.uint64)
        hs.rs_site(site, idx, l.ctypes.data_as(pd), h.ctypes.data_as(pd), out.ctypes.data_as(p64), n)
        assert (out == want).all(), site
    hs.rs_wrap_runs(runs, 1)
    assert runs[0] >= 2 * 13 and runs[2] >= 13 and runs[1] == 0


# ---- the b block ----------------------------------------------------------------------------------------------------------------
def mat(hs, which):
    buf = (ctypes.c_double * 36)()
    n = hs.rs_matrix(which, buf)
    v = [Fraction(x) for x in buf[:n]]
    return [v[6 * i:6 * i + 6] for i in range(6)] if n == 36 else v


def mm(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(6)) for j in range(6)] for i in range(6)]


def test_b_block_matrices_against_the_dense_ones(hs):
    K = [[Fraction(v) for v in row] for row in AC.K_B]
    T = [[Fraction(int(i == j)) for j in range(6)] for i in range(6)]
    T[0][4] = T[1][5] = Fraction(-1)
    T[2][4] = T[3][5] = Fraction(1)
    Ti = [[2 * int(i == j) - T[i][j] for j in range(6)] for i in range(6)]
    assert mm(T, Ti) == [[int(i == j) for j in range(6)] for i in range(6)]
    assert mat(hs, 0) == K and mat(hs, 1) == mm(K, K) and mat(hs, 4) == T and mat(hs, 5) == Ti
    KT = mm(mm(T, K), Ti)
    KT2 = mm(KT, KT)
    assert mat(hs, 2) == KT and mat(hs, 3) == KT2 == mm(mm(T, mm(K, K)), Ti) == mat(hs, 8)
    # the numbers of the change: the 4 x 4 block, the two dense rows, 28 non-zeros, the functionals
    assert [r[:4] for r in KT2[:4]] == [[-864, 360, -1296, 432], [-72, -864, 360, -1296], [1296, -432, 432, -72], [-360, 1296, -432, 432]]
    assert KT2[4:] == [[972, -504, 324, 72, 756, -720], [144, 972, -504, 324, 720, 756]]
    assert all(v == 0 for r in KT2[:4] for v in r[4:]) and sum(v != 0 for r in KT2 for v in r) == 28
    assert mat(hs, 6) == [4, 2, 2, -2, -30, 12] and mat(hs, 7) == [3, -3, 15, 0, -1, -1]
    assert max(sum(abs(v) for v in r) for r in KT2) == 3420


def test_one_trip_against_the_dense_form(hs):
    """single planes exactly (the basis change commutes with the squared layer and with both functionals), then a whole trip on both
    planes with its normalisation: the same values mod p, component by component, through the basis change"""
    rng = np.random.default_rng(77)
    T = mat(hs, 4)

    def dom(op, s):
        a = (ctypes.c_double * 13)(*[float(x) for x in s])
        y = (ctypes.c_double * 12)()
        hs.rs_dom(op, a, y)
        return [Fraction(v) for v in y]

    def to_tri(v):
        return v[:6] + [sum(T[i][j] * v[6 + j] for j in range(6)) for i in range(6)]
    for _ in range(100):
        u = [Fraction(int(x)) for x in rng.integers(-AC.LIM, AC.LIM, 12)]
        d = Fraction(int(rng.integers(-AC.DOM_D_BOUND, AC.DOM_D_BOUND)))
        ut = to_tri(u)
        assert dom(4, u + [0]) == ut and dom(5, ut + [0]) == u
        assert dom(0, ut + [d]) == to_tri(dom(2, u + [d])) == to_tri(AC.dom_exact(6, u + [d]))
        assert dom(1, ut + [0])[0] == dom(3, u + [0])[0] == AC.dom_exact(7, u + [0])[0]
        assert dom(6, ut + [0])[0] == u[0] + u[3] + u[6]
    U = AC.U
    val = lambda l, h: (l + h * (1 << 32)) / U       # the field value of a limb pair of planes in units of 2^32 (an integer, or quarters)
    for _ in range(100):
        wl = [Fraction(int(x)) * U for x in rng.integers(-(1 << 47), 1 << 47, 12)]
        wh = [Fraction(int(x)) * U for x in rng.integers(-(1 << 47), 1 << 47, 12)]
        d1 = [Fraction(int(x)) * U for x in rng.integers(-(1 << 49), 1 << 49, 2)]
        d2 = [Fraction(int(x)) * U for x in rng.integers(-(1 << 41), 1 << 41, 2)]
        res = []
        for tri, (a, b) in ((0, (wl, wh)), (1, (to_tri(wl), to_tri(wh)))):
            out = (ctypes.c_double * 26)()
            hs.rs_trip(tri, (ctypes.c_double * 12)(*map(float, a)), (ctypes.c_double * 12)(*map(float, b)), (ctypes.c_double * 2)(*map(float, d1)),
                       (ctypes.c_double * 2)(*map(float, d2)), out)
            o = [Fraction(v) for v in out]
            res.append(([val(o[k], o[12 + k]) for k in range(12)], val(o[24], o[25])))
        (dense, zd), (tri_, zt) = res
        want = to_tri(dense)
        assert all(x.denominator == 1 for x in want + tri_ + [zd, zt])
        assert [int(x) % P for x in want] == [int(x) % P for x in tri_] and int(zd) % P == int(zt) % P


def test_magnitudes_in_the_triangular_basis(hs):
    """test_hostsim.py::test_double_precision_magnitudes replayed with the b block in the basis of the rounds: the bounds of a plane are
    those of the aa block as before — the b block's own, one bit more for B2, B3 included, stay far inside — and every limb that
    reaches `recombine_s` is within the range its margins were derived from."""
    import gen_tables as G
    lim, n = AC.LIM, 1 << 32
    KT2 = mat(hs, 3)
    cz_b, kt_b = mat(hs, 6), mat(hs, 7)
    cz = 64 + 64 + 128 + 4 + 8 + 32 + int(sum(abs(v) for v in cz_b))
    assert cz == 352                                       # 350 dense
    k2_b = int(max(sum(abs(v) for v in r) for r in KT2))
    kt = max(32, int(max(abs(v) for v in kt_b)))
    assert k2_b == 3420 and kt == 32
    k2 = max(4096 * 16, (4 + 8 + 32) ** 2, k2_b)
    assert k2 == 1 << 16                                   # the aa block stays the bound
    plo, phi = G.PARTIAL_LIMBS
    x = 64 * 4 * n
    xb = 2 * 25 * 2 * n                                    # b products at the entry (unscaled rows sum to 25, inputs sum two limbs), B2 / B3 add two
    for trip in range(11):
        z = 3 * x + xb + 8 * n                             # element 0 reads four entries now: E0 + F0 + B0 + u4
        assert plo <= -z and z <= phi
        w = max(x, xb) + (n + z)
        assert w * 4 < 1 << 53
        z2 = cz * lim + 8 * n
        assert plo <= -z2 and z2 <= phi
        x = k2 * lim + kt * (n + z2)
        xb = k2_b * lim + kt * (n + z2)
        assert xb < x < 1 << 53
    # leaving: u2 = B2 - u4, u3 = B3 - u5 (two b components), then T^-1' adds four products, + the diagonal
    assert 2 * x + 2 * (2 * xb) + 8 * n <= phi
    assert 4 * x + 8 * n < (1 << 51) - (1 << 32)           # the bound of the dense form, for comparison
    # a full-round layer: 32-bit limbs through the circulant (entries sum to 256) and the diagonal 8
    assert (sum(AC.MDS_C) + 8) * EPS == G.FULL_LIMBS[1]


# ---- the permutation ------------------------------------------------------------------------------------------------------------
def run(lib, st, form):
    out = st.copy()
    assert lib.rs_permute(out.ctypes.data_as(p64), out.shape[0], form) == 0
    return out


@pytest.mark.parametrize("form", [PERMUTE, ABSORB, SQUEEZE, NODE], ids=["permute", "permute_absorb", "permute_squeeze", "permute_node"])
def test_permutation_forms_equal_textbook_and_oracle(hs, hs_v1, form):
    st = AC.input_states()
    ref_in = st.copy()
    if form == NODE:
        ref_in[:, 8:] = 0
        st[1::2, 8:] = np.uint64(0xDEADBEEFDEADBEEF)
        st[::2, 8:] = 0
    want = run(hs, ref_in, TEXTBOOK)
    assert (want == O.permute_many(ref_in % np.uint64(P)).reshape(-1, 12)).all()
    live, canonical = LIVE[form]
    for lib in (hs, hs_v1):
        got = run(lib, st, form)
        if canonical:
            assert (got[:, live] == want[:, live]).all()
        else:
            assert ((got[:, live] % np.uint64(P)) == want[:, live]).all()


def test_17_chained_absorbs(hs):
    n = 24
    chunks = AC.absorb_chunks(n)
    a = np.zeros((n, 12), np.uint64)
    b = a.copy()
    for c in range(17):
        a[:, :8] = chunks[c]
        b[:, :8] = chunks[c]
        a = run(hs, a, ABSORB)
        b = run(hs, b, TEXTBOOK)
        assert ((a[:, 8:] % np.uint64(P)) == b[:, 8:]).all(), c
    b2 = np.zeros((n, 12), np.uint64)
    for c in range(17):
        b2[:, :8] = chunks[c] % np.uint64(P)
        b2 = O.permute_many(b2).reshape(-1, 12)
    assert (b == b2).all()


def test_seeded_states_take_the_rare_path(hs):
    """the states of the device test (tests/test_gpu_recombine_small_top.py, k_permute): the repair runs in a partial round and at
    the exit of the partial rounds; a full-round layer (top word <= 266) does not wrap for this seed — its repair is driven by the
    diagnostic entry there"""
    st = RC.permute_states()
    runs = (ctypes.c_ulonglong * 3)()
    hs.rs_wrap_runs(runs, 1)
    got = run(hs, st, PERMUTE)
    hs.rs_wrap_runs(runs, 1)
    assert (got == O.permute_many(st).reshape(-1, 12)).all()
    assert runs[1] >= 1 and runs[2] >= 1, list(runs)
    assert runs[0] == 0, list(runs)
