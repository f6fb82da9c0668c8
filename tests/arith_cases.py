"""Operand tables of the arithmetic unit tests, shared by the CPU tests (hostsim: tests/test_hostsim.py, tests/test_renorm_units.py,
tests/test_air.py) and their device twins (tests/test_gpu_devsim.py), with the exact references they are held against: Python
integers and Fractions only. Pure Python, no GPU, no library."""
import itertools
from fractions import Fraction

import numpy as np

import oracle_lib as O
import rare_paths as R

P = O.P
M64 = (1 << 64) - 1
EPS = 0xFFFFFFFF

# ---- gl.h ---------------------------------------------------------------------------------------------------------------------
GL_EDGE = [0, 1, P - 1, P, M64]
GL_EDGE_PAIRS = list(itertools.product(GL_EDGE, repeat=2))
POW_BASES = [0, 1, P - 1, 7]
POW_EXPONENTS = [0, 1, 2, 7, P - 2, P - 1, M64]
LAZY_EXTREMES = [0, 1, P - 1, P, P + 1, M64, M64 - 1, M64 - EPS, 1 << 63, 0xFFFFFFFF00000000, EPS, EPS + 1]
MUL_ADD_C = [0, 1, (1 << 32) - 1, (1 << 64) - (1 << 32), M64]


def lazy_operands(n, seed):
    """n pairs in [p, 2^64)^2, the bounds first"""
    rng = np.random.default_rng(seed)
    a = rng.integers(P, 1 << 64, n, dtype=np.uint64)
    b = rng.integers(P, 1 << 64, n, dtype=np.uint64)
    for i, (x, y) in enumerate(itertools.product([P, P + 1, M64 - 1, M64], repeat=2)):
        a[i], b[i] = x, y
    return a, b


def mul_add_cases(pairs):
    """(a, b, c): every pair with every c of MUL_ADD_C and the four c around the wrap of lo + c, lo the low half of a b"""
    out = []
    for a, b in pairs:
        lo = (int(a) * int(b)) & M64
        cs = list(MUL_ADD_C) + [(-lo) & M64, (-lo - 1) & M64, (-lo + 1) & M64, (M64 - lo)]
        out += [(int(a), int(b), c) for c in cs]
    return out


def reduce128_cases():
    """(lo, hi, cy): direct tables for reduce128_lazy. hi is the TRUE high half; cy = 1 rows are valid for the three-argument form
    only (they need hi32(hi) >= 1: the carry is part of it). Among them lo < hi32(hi) (borrow repair), lo == hi32(hi) - cy corners,
    and lo32(hi) = 2^32 - 1 with t0 near 2^64 (fold wrap)."""
    los = [0, 1, 2, EPS - 1, EPS, EPS + 1, (1 << 33) - 1, P - 1, P, M64 - EPS, M64 - 1, M64, 1 << 63]
    w2s = [0, 1, 1 << 31, EPS - 1, EPS]
    w3s = [0, 1, 2, 1 << 31, EPS - 1, EPS]
    out = []
    for lo, w2, w3 in itertools.product(los, w2s, w3s):
        out.append((lo, (w3 << 32) | w2, 0))
        if w3:
            out.append((lo, (w3 << 32) | w2, 1))
    for w3 in w3s[1:]:                      # lo around w3: borrows by one, meets it, clears it
        for lo in (w3 - 1, w3, w3 + 1):
            for w2 in (0, EPS):
                out += [(lo, (w3 << 32) | w2, 0), (lo, (w3 << 32) | w2, 1)]
    rng = np.random.default_rng(21)
    for _ in range(200):
        lo, hi = (int(v) for v in rng.integers(0, 1 << 64, 2, dtype=np.uint64))
        out.append((lo, hi, int(hi >> 32 != 0 and rng.integers(0, 2))))
    return out


def fold_top_cases():
    """(lo, top): top in {0, 1, 2^32 - 1} (and one in between), lo just below, at and just above the value at which
    lo + top (2^32 - 1) wraps 2^64"""
    out = []
    for top in (0, 1, 1 << 31, EPS):
        thr = (1 << 64) - top * EPS
        for lo in (0, 1, thr - 2, thr - 1, thr, thr + 1, M64 - 1, M64, P):
            if 0 <= lo <= M64:
                out.append((lo, top))
    return out


def fold_top_py(lo, top):
    s = lo + top * EPS
    return (s + EPS) & M64 if s >> 64 else s


# ---- ntt16.h ------------------------------------------------------------------------------------------------------------------
MUL_POW2_SHIFTS = (0, 1, 5, 12, 24, 31, 32, 33, 36, 48, 60, 63, 64, 65, 72, 84, 95)
MUL_POW2_EDGE = [0, 1, P - 1, P - 2, 0xFFFFFFFF, 0xFFFFFFFF00000000, 1 << 63]


def mul_pow2_operands():
    rng = np.random.default_rng(2)
    return [int(x) % P for x in rng.integers(0, 2**64, 200, dtype=np.uint64)] + MUL_POW2_EDGE


def round16_inputs():
    x = O.splitmix64_felts(5, 16)
    x[0], x[1], x[2] = P - 1, 0, 1
    return x


# ---- poseidon.h: the permutation forms ----------------------------------------------------------------------------------------
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


def absorb_chunks(n=24):
    """the 17 rate chunks of a 135-column leaf for n sponges, boundary chunks among them"""
    chunks = O.splitmix64_felts(0xAB50, 17 * n * 8).reshape(17, n, 8).copy()
    chunks[2] = P - 1
    chunks[5] = 0
    chunks[9] = M64
    return chunks


# ---- poseidon.h: the normalisation against exact rationals ----------------------------------------------------------------------
U = Fraction(1, 1 << 32)            # one old unit in the new ones
LIM = (1 << 31) + (1 << 20)         # a normalised limb, old units (the magnitude comment above dom_mul_d)
BOUND = 1 << 50                     # above every limb entering the normalisation (2^49.3, old units), two fractional bits included


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


RECOMBINE_LIM = (1 << 51) - (1 << 32) - 1       # recombine_d's range


def recombine_limbs():
    rng = np.random.default_rng(12)
    lim = RECOMBINE_LIM
    return [(0, 0), (lim, lim), (-lim, -lim), (lim, -lim), (-1, 0), (0, -1), (1, 1)] + [tuple(int(v) for v in rng.integers(-lim, lim, 2)) for _ in range(40)]


# the conversion at its limits (c as hs_recombine_d takes it: the constant, stored minus the offset B (1 + 2^32))
RECOMBINE_OFFSET = ((0x433 << 52) + (1 << 51)) * (1 + (1 << 32))
RECOMBINE_CONST_CASES = ((0, 0, 0), ((1 << 51) - (1 << 32) - 1, (1 << 51) - (1 << 32) - 1, P - 1), (-(1 << 51) + 1, -(1 << 51) + 1, 5), (-1, 0, 0), (0, -1, 0),
                         (123456789012345, -98765432109876, 0xFFFFFFFF00000000))

# ---- poseidon.h: the layers of the transformed domain ----------------------------------------------------------------------------
MDS_C = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]


def dom_vectors():
    """the integer planes of test_double_precision_layer_identities (drawn first from its generator)"""
    rng = np.random.default_rng(4)
    return rng, [[int(x) for x in rng.integers(-(1 << 40), 1 << 40, 12)] for _ in range(200)]


def lazy_states(rng):
    return [[0] * 12, [M64] * 12, [P - 1] * 12, [M64, 0] * 6] + [[int(x) for x in rng.integers(0, 1 << 64, 12, dtype=np.uint64)] for _ in range(300)]


def mds_py(st):
    return [(sum(MDS_C[i] * st[(i + r) % 12] for i in range(12)) + (8 * st[0] if r == 0 else 0)) % P for r in range(12)]


# The scaled layer K (dom_mul_d<true>) as a matrix over the index layout [0..2] = aa, [3..5] = ab, [6..11] = b, restated from the
# comment of poseidon.h: aa = 64 (J + P), P: row i takes column (i + 2) % 3
K_AA = [[64 + 64 * (j == (i + 2) % 3) for j in range(3)] for i in range(3)]
K_AB = [[-4, -8, 32], [-32, -4, -8], [8, -32, -4]]
K_B = [[4, 2, 2, -2, -32, 8], [-8, 4, 2, 2, -2, -32], [32, -8, 4, 2, 2, -2], [2, 32, -8, 4, 2, 2], [-2, 2, 32, -8, 4, 2], [-2, -2, 2, 32, -8, 4]]


def _block_diag(*blocks):
    n = sum(len(b) for b in blocks)
    m = [[0] * n for _ in range(n)]
    at = 0
    for b in blocks:
        for i, row in enumerate(b):
            for j, v in enumerate(row):
                m[at + i][at + j] = v
        at += len(b)
    return m


DOM_K = _block_diag(K_AA, K_AB, K_B)
DOM_K2 = [[sum(DOM_K[i][k] * DOM_K[k][j] for k in range(12)) for j in range(12)] for i in range(12)]
DOM_KT = [Fraction(DOM_K[i][(0, 3, 6)[(i >= 3) + (i >= 6)]], (4, 4, 2)[(i >= 3) + (i >= 6)]) for i in range(12)]   # K t: a change of element 0, one layer on
DOM_CZ = [DOM_K[0][j] + DOM_K[3][j] + DOM_K[6][j] for j in range(12)]                                               # l K: element 0 of the next layer
# what |new - z| of a partial round is bounded by (tests/test_hostsim.py::test_double_precision_magnitudes: n + z2), units of 1
DOM_D_BOUND = (1 << 32) + 350 * LIM + 8 * (1 << 32)


def worst_case_vectors():
    """[(op of sim::dom_d, 13 inputs as Fractions, component, exact value)]: for every output component of dom_mul_d<true> (op 2),
    dom_mul2_d (op 6) and dom_next_z (op 7) the input whose every entry is +-LIM (the bound of a normalised limb; the change d of
    dom_mul2_d at +-DOM_D_BOUND) with the signs of that component's coefficients, and its negation — in units of 1 and scaled by
    2^-32. The component then is the sum of the absolute values: the largest magnitude the layer can produce."""
    out = []
    rows = [(2, DOM_K[i] + [0], i) for i in range(12)] + [(6, [Fraction(v) for v in DOM_K2[i]] + [DOM_KT[i]], i) for i in range(12)] + [(7, DOM_CZ + [0], 0)]
    for op, coef, comp in rows:
        for sign in (1, -1):
            for unit in (Fraction(1), U):
                s = [Fraction(sign * ((c > 0) - (c < 0)) * (DOM_D_BOUND if j == 12 else LIM)) * unit for j, c in enumerate(coef)]
                if op != 6:
                    s[12] = Fraction(0)
                want = sum(Fraction(c) * v for c, v in zip(coef, s))
                assert abs(want) == sum(abs(Fraction(c) * v) for c, v in zip(coef, s))
                out.append((op, s, comp, want))
    return out


def dom_exact(op, s):
    """all twelve outputs of ops 2, 6, 7 on Fractions"""
    if op == 2:
        return [sum(Fraction(DOM_K[i][j]) * s[j] for j in range(12)) for i in range(12)]
    if op == 6:
        return [sum(Fraction(DOM_K2[i][j]) * s[j] for j in range(12)) + DOM_KT[i] * s[12] for i in range(12)]
    return [sum(Fraction(DOM_CZ[j]) * s[j] for j in range(12))] + [Fraction(0)] * 11


# ---- ext3.h -------------------------------------------------------------------------------------------------------------------
def cubic_mul_py(m, a, b):
    """(a0 + a1 X + a2 X^2)(b0 + b1 X + b2 X^2) mod X^3 - m1 X - m0"""
    c = [0] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] += a[i] * b[j]
    for k in (4, 3):                       # X^k = m1 X^(k - 2) + m0 X^(k - 3)
        c[k - 2] += m[1] * c[k]
        c[k - 3] += m[0] * c[k]
    return tuple(v % P for v in c[:3])


def cubic_norm_py(m, a):
    """det of the multiplication-by-a matrix (columns a, X a, X^2 a)"""
    c0 = a
    c1 = cubic_mul_py(m, a, (0, 1, 0))
    c2 = cubic_mul_py(m, c1, (0, 1, 0))
    M = [[c0[i], c1[i], c2[i]] for i in range(3)]
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])) % P


REDUCIBLE_MODULUS = (0, 5)                 # X^3 - 5 X = X (X^2 - 5): X, X^2 - 5 and their multiples have norm 0
ZERO_NORM_ELEMENTS = [(0, 1, 0), (0, 0, 1), (P - 5, 0, 1), (0, 7, 0), (0, 3, 11)]


def cubic_moduli(rng):
    import air_programs as A
    return (A.CUBIC_MODULUS, (1, 1), (5, 0), (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64))))


def cubic_cases():
    """[(m, a, b)] of test_cubic_and_prefix_sum_primitives, in its order of drawing, then the reducible modulus with its zero-norm elements"""
    rng = np.random.default_rng(2)
    out = []
    for m in cubic_moduli(rng):
        for _ in range(20):
            a = tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64))
            b = tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64))
            out.append((m, a, b))
        rng.integers(0, P, (6, 17), dtype=np.uint64)      # the columns the CPU test draws here
    rng = np.random.default_rng(22)
    for a in ZERO_NORM_ELEMENTS + [(0, 0, 0), (1, 0, 0), (P - 1, P - 1, P - 1)]:
        b = tuple(int(v) for v in rng.integers(0, P, 3, dtype=np.uint64))
        out.append((REDUCIBLE_MODULUS, a, b))
    return out


# ---- BLS12-381 (bls12_381.h, bls12_381_fr.h): the value tables of tests/test_hostsim.py --------------------------------------------
def bls_fp_values():
    p, r, G = O.bls_constants()
    rng = np.random.default_rng(4)
    return [0, 1, 2, p - 1, p - 2, (1 << 380) + 12345, G[0], G[1]] + [int.from_bytes(rng.bytes(48), "little") % p for _ in range(40)]


def bls_loose_values():
    """(values below 32 p for the loose primitives, the generator they were drawn from)"""
    p, r, G = O.bls_constants()
    rng = np.random.default_rng(14)
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 8 * p, 16 * p - 1, 16 * p, 22 * p - 1, 31 * p, 32 * p - 1]
    vals += [int.from_bytes(rng.bytes(49), "little") % (32 * p) for _ in range(40)]
    return vals, rng


def bls_fr_values():
    """(values of the scalar field, the generator they were drawn from)"""
    _, r, _ = O.bls_constants()
    rng = np.random.default_rng(12)
    return [0, 1, 2, r - 1, r - 2, (1 << 254) + 99, 7] + [int.from_bytes(rng.bytes(32), "little") % r for _ in range(40)], rng


def bls_fp2_pairs(count=20):
    p, _, _ = O.bls_constants()
    rng = np.random.default_rng(6)
    draw = lambda: (int.from_bytes(rng.bytes(48), "little") % p, int.from_bytes(rng.bytes(48), "little") % p)
    return [(draw(), draw()) for _ in range(count)], rng


GROUP_SMALL_K = (0, 1, 2, 3, 255, 65535, 40000)


def bls_g1_points():
    p, r, G = O.bls_constants()
    rng = np.random.default_rng(5)
    return [O.bls_g1_mul(G, int.from_bytes(rng.bytes(32), "little") % r) for _ in range(5)] + [G]


def bls_g2_points(rng):
    """drawn after bls_fp2_pairs from the same generator, as the CPU test does"""
    _, r, _ = O.bls_constants()
    G2 = O.bls_g2_generator()
    return [O.bls_g2_mul(G2, int.from_bytes(rng.bytes(32), "little") % r) for _ in range(3)] + [G2]


def bls_bucket_scalars():
    _, r, _ = O.bls_constants()
    rng = np.random.default_rng(15)
    return [int.from_bytes(rng.bytes(32), "little") % r for _ in range(40)]
