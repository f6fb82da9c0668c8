"""The partial rounds of the permutation keep their limb planes in units of 2^32 (poseidon.h `renorm32_d`: the carry is one
rint): the four permutation forms against `permute_textbook` and the oracle, the normalisation alone against exact rational
arithmetic, and the constants of the scaled planes against the unscaled ones through `recombine_d`. CPU only."""
import ctypes
import os
import re
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "renorm_hostsim"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "city-rollup_amd", "csrc")
P = O.P
M64 = (1 << 64) - 1
p64 = ctypes.POINTER(ctypes.c_uint64)
pd = ctypes.POINTER(ctypes.c_double)
PERMUTE, ABSORB, SQUEEZE, NODE, TEXTBOOK = range(5)
# form -> (live words, canonical on exit)
LIVE = {PERMUTE: (slice(0, 12), True), ABSORB: (slice(8, 12), False), SQUEEZE: (slice(0, 4), True), NODE: (slice(0, 4), True)}
U = Fraction(1, 1 << 32)            # one old unit in the new ones
LIM = (1 << 31) + (1 << 20)         # a normalised limb, old units (the magnitude comment above dom_mul_d)
BOUND = 1 << 50                     # above every limb entering the normalisation (2^49.3, old units), two fractional bits included


@pytest.fixture(scope="module")
def hs():
    import renorm_hostsim_build as hb
    lib = ctypes.CDLL(hb.build())
    lib.hs_rn_renorm.argtypes = [ctypes.c_int, pd, pd]
    lib.hs_rn_recombine.restype = ctypes.c_uint64
    lib.hs_rn_recombine.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    lib.hs_rn_permute.argtypes = [p64, ctypes.c_size_t, ctypes.c_int]
    assert lib.hs_rn_units32() == 1, "the default build keeps the partial rounds in units of 2^32"
    return lib


# ---- the permutation forms ------------------------------------------------------------------------------------------
def input_states():
    """random canonical states, all zero, all p - 1, rows of boundary words, lazy words at 2^64 - 1 (capacity only, everywhere)"""
    rng = np.random.default_rng(31)
    st = O.splitmix64_felts(0x2E4032, 12 * 160).reshape(-1, 12).copy()
    st[0] = 0
    st[1] = P - 1
    st[2] = M64
    st[3, 8:] = M64
    edge = np.array([0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 1 << 63, M64, M64 - 0xFFFFFFFF, P, P + 1],
                    np.uint64)
    for i in range(4, 64):
        st[i] = rng.choice(edge, 12)
    return st


def run(hs, st, form):
    out = st.copy()
    assert hs.hs_rn_permute(out.ctypes.data_as(p64), out.shape[0], form) == 0
    return out


@pytest.mark.parametrize("form", [PERMUTE, ABSORB, SQUEEZE, NODE], ids=["permute", "permute_absorb", "permute_squeeze", "permute_node"])
def test_permutation_forms_equal_textbook_and_oracle(hs, form):
    st = input_states()
    ref_in = st.copy()
    if form == NODE:                 # a tree node declares its capacity zero: what the words hold is never read
        ref_in[:, 8:] = 0
        st[1::2, 8:] = np.uint64(0xDEADBEEFDEADBEEF)
        st[::2, 8:] = 0
    want = run(hs, ref_in, TEXTBOOK)
    assert (want == O.permute_many(ref_in % np.uint64(P)).reshape(-1, 12)).all()
    got = run(hs, st, form)
    live, canonical = LIVE[form]
    if canonical:
        assert (got[:, live] == want[:, live]).all()
    else:
        assert ((got[:, live] % np.uint64(P)) == want[:, live]).all()


def test_17_chained_absorbs(hs):
    """the middle of a 135-column leaf: 17 capacity-only permutations, the lazy capacity carried from one to the next"""
    n = 24
    chunks = O.splitmix64_felts(0xAB50, 17 * n * 8).reshape(17, n, 8).copy()
    chunks[2] = P - 1
    chunks[5] = 0
    chunks[9] = M64
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


# ---- the normalisation alone, against exact rationals ------------------------------------------------------------------
def rne(x):
    """round to nearest, ties to even (what rint does in the default rounding mode)"""
    f = x.numerator // x.denominator
    r = x - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2):
        f += 1
    return f


def representable(x):
    return Fraction(float(x)) == x


def exact_renorm32(L, H):
    """renorm32_d step by step in exact arithmetic; every intermediate must be a double (then no operation rounds: an IEEE
    operation whose exact result is representable returns it)"""
    c = rne(L)
    l1 = L - c
    h1 = H + c * U
    t = rne(h1)
    h2 = h1 - t * (1 - U)
    l2 = l1 - t * U
    steps = (Fraction(c), l1, h1, Fraction(t), h2, l2)
    assert all(representable(s) for s in steps), (L, H, steps)
    return l2, h2, c, t


def renorm_cases():
    """(l, h) in OLD units (value l + 2^32 h), Fractions with denominators up to 4"""
    rng = np.random.default_rng(8)
    B, T31, T32 = BOUND, 1 << 31, 1 << 32
    cases = []
    q = lambda a, b=0: Fraction(4 * a + b, 4)
    # the bounds of the magnitude comment: just inside 2^50, two fractional bits
    for l in (q(B - 1, 3), q(-B + 1, -3), q(0), q(1), q(-1), q(0, 1), q(0, -1)):
        for h in (q(B - 1, 3), q(-B + 1, -3), q(0), q(1), q(-1)):
            cases.append((l, h))
    # quarter-integer limbs
    for _ in range(1500):
        l, h = (int(v) for v in rng.integers(-B + 1, B - 1, 2))
        cases.append((q(l, int(rng.integers(0, 4))), q(h, int(rng.integers(0, 4)))))
    # every tie: l an odd multiple of 2^31 (c decides between two even / odd neighbours), h likewise once c / 2^32 has gone in
    for k in list(range(-9, 10, 2)) + [(1 << 18) - 1, -(1 << 18) + 1, (1 << 19) - 3, 54321]:
        cases.append((Fraction(k * T31), Fraction(0)))
        cases.append((Fraction(0), Fraction(k * T31)))
        cases.append((Fraction(k * T31), Fraction((k + 2) * T31)))
        c = rne(Fraction(k, 2))
        cases.append((Fraction(k * T31), Fraction(3 * T31 - c)))   # h + c lands exactly on a tie of the second rounding
    # carries: c != 0 and t != 0 with all four sign combinations, small and large
    for cs in (1, -1):
        for ts in (1, -1):
            for cm, tm in ((1, 1), (3, 2), (1 << 17, 1 << 17), ((1 << 18) - 1, (1 << 18) - 1)):
                cases.append((Fraction(cs * cm * T32 + cs * 5), Fraction(ts * tm * T32 + ts * 7)))
                cases.append((q(cs * cm * T32, cs * 1), q(ts * tm * T32 + ts * (T31 - 1), ts * 3)))
    return cases


def test_renorm32_against_exact_rationals(hs):
    cases = renorm_cases()
    seen = set()
    ties = 0
    for l, h in cases:
        assert abs(l) < BOUND and abs(h) < BOUND
        L, H = l * U, h * U
        assert representable(L) and representable(H)
        wl, wh, c, t = exact_renorm32(L, H)
        seen.add((c > 0) - (c < 0) if t == 0 else ((c > 0) - (c < 0), (t > 0) - (t < 0)))
        ties += (L - (L.numerator // L.denominator) == Fraction(1, 2)) + ((H + c * U) - ((H + c * U).numerator // (H + c * U).denominator) == Fraction(1, 2))
        arr = (ctypes.c_double * 2)(float(L), float(H))
        out = (ctypes.c_double * 2)()
        hs.hs_rn_renorm(0, arr, out)
        assert (Fraction(out[0]), Fraction(out[1])) == (wl, wh), (l, h)
        # within the stated bound, old units
        assert abs(wl) <= LIM * U and abs(wh) <= LIM * U, (l, h, out[0], out[1])
        # the value mod p: (l + 2^32 h) moves by -t (2^64 - 2^32 + 1)
        d = ((wl + (1 << 32) * wh) - (L + (1 << 32) * H)) / U
        assert d.denominator == 1 and d.numerator % P == 0 and d.numerator == -t * P, (l, h)
        # the same limbs as the two-operation form in units of 1, scaled (ties included: both round to nearest-even)
        arr1 = (ctypes.c_double * 2)(float(l), float(h))
        out1 = (ctypes.c_double * 2)()
        hs.hs_rn_renorm(1, arr1, out1)
        assert (Fraction(out1[0]) * U, Fraction(out1[1]) * U) == (wl, wh), (l, h)
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1)} <= seen, "a sign combination of the two carries was not reached"
    assert ties >= 40, "the tie cases did not land on ties"


# ---- the constants of the scaled planes ---------------------------------------------------------------------------------
def parse_table(name):
    src = open(os.path.join(CSRC, "poseidon_tables.h")).read()
    m = re.search(r"%s\[\d+\] = \{(.*?)\};" % name, src, re.S)
    return [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)", m.group(1))]


def test_scaled_constants_reproduce_the_unscaled_integers(hs):
    """POSEIDON_DOMD32_* hold each constant as 1.5 * 2^20 + half * 2^-32, minus the bit pattern of 1.5 * 2^20 at both limb positions:
    decoded they are the constants gen_tables.py derives, and through `recombine_d` a scaled limb pair with a scaled entry gives the
    very u64 that the unscaled pair gives with the unscaled entry."""
    sys.path.insert(0, CSRC)
    import gen_tables
    dk, dlast = gen_tables.plane_constants(gen_tables.round_constants(), first_too=True)
    B32 = (0x413 << 52) + (1 << 51)
    rng = np.random.default_rng(12)
    lim = (1 << 51) - (1 << 32) - 1       # recombine_d's range
    limbs = [(0, 0), (lim, lim), (-lim, -lim), (lim, -lim), (-1, 0), (0, -1), (1, 1)] + [tuple(int(v) for v in rng.integers(-lim, lim, 2)) for _ in range(40)]
    for name, want, t_old, t_new in (("POSEIDON_DOMD32_K", dk, 0, 2), ("POSEIDON_DOMD32_LAST", dlast, 1, 3)):
        got = parse_table(name)
        assert len(got) == 2 * len(want)
        for i, c in enumerate(want):
            halves = []
            for bits in got[2 * i:2 * i + 2]:
                d = Fraction(struct.unpack("<d", struct.pack("<Q", bits))[0]) - 3 * (1 << 19)
                h = d / U
                assert h.denominator == 1 and 0 <= h < (1 << 32)
                assert bits == B32 + int(h)        # the mantissa holds the half; the exponent field is that of 1.5 * 2^20
                halves.append(int(h))
            assert (halves[0] + (halves[1] << 32) + B32 * (1 + (1 << 32))) % P == c
            for l, h in limbs:
                a = hs.hs_rn_recombine(float(l), float(h), t_old, i)
                b = hs.hs_rn_recombine(float(Fraction(l) * U), float(Fraction(h) * U), t_new, i)
                assert a == b, (name, i, l, h)
                assert a % P == (l + (h << 32) + c) % P

