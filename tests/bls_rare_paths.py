"""Inputs that take the rare paths of the BLS12-381 arithmetic (csrc/bls12_381_fr.h, bls12_381.h, r1cs.h) on purpose, and the
witnesses that they do. Pure Python, no GPU; the sibling of tests/rare_paths.py, whose lane `patterns` it reuses.

Restated with Python integers: the Montgomery product scan before its final subtraction (`mont_t`, `scan`), the loose
primitives (`lz_*`), `mul_small` with its quotient estimate and the number of subtractions it takes, and
`xyzz_add_mixed_loose` for both coordinate fields with the way it went. Constructed against them: F_r operands whose product with
a KNOWN second operand needs the final subtraction (`plant_fr`), curve points that pass the 28-bit "same x?" filter without
having the same x, families of them, points whose Montgomery x has saturated limbs, and the inputs of every case of
tests/test_gpu_bls_rare_paths.py together with the operand pairs that witness the planted path; tests/test_bls_rare_paths.py
calls all of it on the CPU."""
import collections

import numpy as np

from rare_paths import patterns, PATTERNS  # noqa: F401  (lane layouts: one vocabulary for both rare-path suites)

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LB = 28
LM = (1 << LB) - 1
FP_NL, FR_NL = 14, 10
RADIX_P, RADIX_R = 1 << (LB * FP_NL), 1 << (LB * FR_NL)      # the Montgomery radices 2^392 and 2^280
P_NINV, R_NINV = pow(-P, -1, RADIX_P), pow(-R, -1, RADIX_R)
RP_INV, RR_INV = pow(RADIX_P, -1, P), pow(RADIX_R, -1, R)
ONE_P, ONE_R = RADIX_P % P, RADIX_R % R                       # Montgomery one
R2_R = RADIX_R * RADIX_R % R                                  # what fr_from_canonical multiplies by
PINV28 = pow(P, -1, 1 << LB)
M64 = (1 << 64) - 1


def limbs(v, n):
    assert 0 <= v < 1 << (LB * n)
    return tuple((v >> (LB * i)) & LM for i in range(n))


def value(l):
    return sum(int(x) << (LB * i) for i, x in enumerate(l))


def rand_below(rng, bound):
    return int.from_bytes(rng.bytes(64), "little") % bound


# ---- the Montgomery product before its final subtraction -----------------------------------------------------------------------
def mont_t(a, b, mod, radix, ninv):
    """T = (a b + m q) / R with m = -a b q^-1 mod R: what the product scan holds before fr_cond_sub / fp_cond_sub_p"""
    ab = a * b
    m = ab * ninv % radix
    return (ab + m * mod) // radix


def fr_t(a, b):
    return mont_t(a, b, R, RADIX_R, R_NINV)


def fp_t(a, b):
    return mont_t(a, b, P, RADIX_P, P_NINV)


def fr_mul(a, b):
    t = fr_t(a, b)
    return t - R if t >= R else t


def fr_subtracts(a, b):
    """fr_mul(a, b) takes its final subtraction (operands as the function sees them: raw values below r)"""
    return fr_t(a, b) >= R


def fp_mul(a, b):
    t = fp_t(a, b)
    return t - P if t >= P else t


def scan(al, bl, mod, nl):
    """the product scan limb by limb, as fr_mul / fp_mul_body run it: (result limbs before the subtraction, the largest value a
    column accumulator held). The accumulator is 64 bits wide: the second number is what must stay below 2^64."""
    ml = limbs(mod, nl)
    n0 = pow(-mod, -1, 1 << LB)
    m, out, acc, top = [0] * nl, [0] * nl, 0, 0
    for k in range(nl):
        acc += sum(al[i] * bl[k - i] for i in range(k + 1)) + sum(m[i] * ml[k - i] for i in range(k))
        m[k] = ((acc & 0xFFFFFFFF) * n0) & LM
        acc += m[k] * ml[0]
        top = max(top, acc)
        assert acc & LM == 0
        acc >>= LB
    for k in range(nl, 2 * nl):
        acc += sum(al[i] * bl[k - i] + m[i] * ml[k - i] for i in range(k - nl + 1, nl))
        top = max(top, acc)
        out[k - nl] = acc & LM
        acc >>= LB
    return tuple(out), top


# ---- F_r operands against a known second operand ---------------------------------------------------------------------------
def _reduce2(u, v):
    """Lagrange-Gauss reduction of a planar lattice basis"""
    n = lambda w: w[0] * w[0] + w[1] * w[1]
    while True:
        if n(u) > n(v):
            u, v = v, u
        d = n(u)
        mu = (2 * (u[0] * v[0] + u[1] * v[1]) + d) // (2 * d)
        if mu == 0:
            return u, v
        v = (v[0] - mu * u[0], v[1] - mu * u[1])


_basis_cache = {}


def plant_fr(b, rng, tries=12):
    """a in (0, r) with fr_subtracts(a, b), for the raw second operand b the kernel will hold; None when the restatement finds none.
    With e = a b r^-1 mod 2^280, T >= r holds exactly when e <= a b / r; the pairs (a, e) are the lattice spanned by
    (1, b r^-1 mod 2^280) and (0, 2^280). Its reduced basis has vectors of about 2^140, the region {0 < a < r, 0 <= e <= a b / r}
    is about 2^255 wide and 2^255 b / r high: a lattice point next to a target drawn inside the region is inside it too."""
    b = int(b)
    if b <= 0:
        return None
    if b not in _basis_cache:
        if len(_basis_cache) > 4096:
            _basis_cache.clear()
        _basis_cache[b] = _reduce2((1, b * pow(R, -1, RADIX_R) % RADIX_R), (0, RADIX_R))
    u, v = _basis_cache[b]
    det = u[0] * v[1] - u[1] * v[0]
    for _ in range(tries):
        a0 = R // 8 + rand_below(rng, R - R // 4)
        hi = a0 * b // R
        if hi < 4:
            return None
        e0 = hi // 4 + rand_below(rng, hi // 2)
        x = (2 * (a0 * v[1] - e0 * v[0]) + det) // (2 * det)
        y = (2 * (u[0] * e0 - u[1] * a0) + det) // (2 * det)
        for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            a = (x + dx) * u[0] + (y + dy) * v[0]
            if 0 < a < R and fr_subtracts(a, b):
                return a
    return None


def plant_fr_load(rng):
    """a canonical input whose conversion fr_from_canonical(a) = fr_mul(a, R^2) subtracts"""
    return plant_fr(R2_R, rng)


def plant_fr_value(b_mont, rng):
    """a canonical VALUE x whose Montgomery form x R subtracts against b_mont (for operands that are converted on load)"""
    a = plant_fr(b_mont, rng)
    return None if a is None else a * RR_INV % R


def fr_mont(x):
    return x * RADIX_R % R


# ---- mul_small (r1cs.h) -------------------------------------------------------------------------------------------------------
SMALL_R1 = R >> 224
MulSmall = collections.namedtuple("MulSmall", "result q_est q n_sub")


def mul_small(w, c):
    """c w mod r the way r1cs::mul_small gets it: the quotient estimated from the bits above 2^224, then conditional subtractions"""
    assert 0 <= w < R and 0 <= c < 1 << LB
    t = w * c
    q_est = (t >> 224) // (SMALL_R1 + 1)
    rem = t - q_est * R
    assert 0 <= rem < RADIX_R
    n_sub = rem // R
    return MulSmall(rem - n_sub * R, q_est, t // R, n_sub)


def mul_small_pairs(rng, count):
    """(one_sub, near_r): count pairs (w, c) each. one_sub needs exactly one conditional subtraction (c w = k r + a remainder below c
    with k large: the estimate is one short); near_r needs none and leaves a remainder just below r (c w = k r - a little)."""
    one, near = [], []
    while len(one) < count or len(near) < count:
        c = (1 << LB) - 1 - rand_below(rng, 1 << 20) if len(one) % 2 else 2 + rand_below(rng, (1 << LB) - 2)
        k = c - 1 - rand_below(rng, max(1, c // 8))
        if k < 1:
            continue
        w_hi, w_lo = -(-k * R // c), k * R // c
        if w_hi < R and mul_small(w_hi, c).n_sub == 1 and len(one) < count:
            one.append((w_hi, c))
        m = mul_small(w_lo, c)
        if m.n_sub == 0 and R - m.result <= c and len(near) < count:
            near.append((w_lo, c))
    return one, near


# ---- loose F_p arithmetic (bls12_381.h), on limb tuples ------------------------------------------------------------------------
def kp_limbs(K):
    return limbs(K * P, FP_NL)


def lz_mul(a, b):
    t = fp_t(value(a), value(b))
    return limbs(t % RADIX_P, FP_NL)


def lz_sqr(a):
    return lz_mul(a, a)


def lz_add_nc(a, b):
    return tuple(x + y for x, y in zip(a, b))


def lz_add(a, b):
    out, c = [], 0
    for x, y in zip(a, b):
        t = x + y + c
        out.append(t & LM)
        c = t >> LB
    return tuple(out)


def lz_sub(K, a, b):
    out, c = [], 0
    for x, y, k in zip(a, b, kp_limbs(K)):
        t = x - y + k + c
        assert -(1 << 31) <= t < 1 << 31, "the signed 32-bit limb difference overflowed"
        out.append(t & LM)
        c = t >> LB
    return tuple(out)


def lz_weak(K, a):
    out, br = [], 0
    for x, k in zip(a, kp_limbs(K)):
        d = (x - k - br) & 0xFFFFFFFF
        out.append(d & LM)
        br = d >> 31
    return tuple(a) if br else tuple(out)


def lz_maybe_zero(a):
    return ((a[0] * PINV28) & LM) < 32


def lz_canon(a):
    return limbs(fp_mul(value(a), ONE_P), FP_NL)


def _is2(a):
    return isinstance(a[0], tuple)


def lf_mul(a, b):
    if not _is2(a):
        return lz_mul(a, b)
    v0, v1 = lz_mul(a[0], b[0]), lz_mul(a[1], b[1])
    s = lz_mul(lz_add_nc(a[0], a[1]), lz_add_nc(b[0], b[1]))
    return (lz_sub(2, v0, v1), lz_sub(4, s, lz_add_nc(v0, v1)))


def lf_sqr(K, a):
    if not _is2(a):
        return lz_sqr(a)
    t = lz_mul(a[0], a[1])
    return (lz_mul(lz_add_nc(a[0], a[1]), lz_sub(K, a[0], a[1])), lz_add(t, t))


def lf_sub(K, a, b):
    return (lz_sub(K, a[0], b[0]), lz_sub(K, a[1], b[1])) if _is2(a) else lz_sub(K, a, b)


def lf_add_nc(a, b):
    return (lz_add_nc(a[0], b[0]), lz_add_nc(a[1], b[1])) if _is2(a) else lz_add_nc(a, b)


def lf_weak(K, a):
    return (lz_weak(K, a[0]), lz_weak(K, a[1])) if _is2(a) else lz_weak(K, a)


def lf_canon(a):
    return (lz_canon(a[0]), lz_canon(a[1])) if _is2(a) else lz_canon(a)


def lf_maybe_zero(a):
    return (lz_maybe_zero(a[0]) and lz_maybe_zero(a[1])) if _is2(a) else lz_maybe_zero(a)


def lf_is_zero(a):
    return not any(a[0]) and not any(a[1]) if _is2(a) else not any(a)


def components(a):
    return list(a) if _is2(a) else [a]


# ---- the canonical field (Montgomery values as integers) for the exact fallback -----------------------------------------------
class _F1:
    one, zero = ONE_P, 0
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b * RP_INV % P)
    to_limbs = staticmethod(lambda a: limbs(a, FP_NL))
    from_limbs = staticmethod(value)


class _F2:
    one, zero = (ONE_P, 0), (0, 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % P, (a[1] + b[1]) % P))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) * RP_INV % P, (a[0] * b[1] + a[1] * b[0]) * RP_INV % P))
    to_limbs = staticmethod(lambda a: (limbs(a[0], FP_NL), limbs(a[1], FP_NL)))
    from_limbs = staticmethod(lambda a: (value(a[0]), value(a[1])))


def xyzz_add_mixed(p, q):
    """bls::xyzz_add_mixed on canonical operands (limb tuples in, limb tuples out) and 'doubling' / 'cancellation' / 'general'"""
    F = _F2 if _is2(q[0]) else _F1
    px, py, pzz, pzzz = (F.from_limbs(c) for c in p)
    qx, qy = F.from_limbs(q[0]), F.from_limbs(q[1])
    u2, s2 = F.mul(qx, pzz), F.mul(qy, pzzz)
    out = lambda *cs: tuple(F.to_limbs(c) for c in cs)
    dbl = lambda a: F.add(a, a)
    if px == u2:
        if py != s2:
            return out(F.one, F.one, F.zero, F.zero), "cancellation"
        u = dbl(qy)
        v = F.mul(u, u)
        w, s, xx = F.mul(u, v), F.mul(qx, v), F.mul(qx, qx)
        m = F.add(dbl(xx), xx)
        x = F.sub(F.mul(m, m), dbl(s))
        return out(x, F.sub(F.mul(m, F.sub(s, x)), F.mul(w, qy)), v, w), "doubling"
    pp_, rr = F.sub(u2, px), F.sub(s2, py)
    pp = F.mul(pp_, pp_)
    ppp, qq = F.mul(pp_, pp), F.mul(px, pp)
    x = F.sub(F.sub(F.mul(rr, rr), ppp), dbl(qq))
    return out(x, F.sub(F.mul(rr, F.sub(qq, x)), F.mul(py, ppp)), F.mul(pzz, pp), F.mul(pzzz, ppp)), "general"


# ---- xyzz_add_mixed_loose ---------------------------------------------------------------------------------------------------------
BOUND = {False: dict(M=2, S=2, X=8, Y=4, WEAK=False), True: dict(M=6, S=4, X=16, Y=12, WEAK=True)}   # LooseBound<Fp>, <Fp2>
WAYS = ("first", "loose", "doubling", "cancellation", "false_positive")   # the codes of hostsim's hs_bls_g*_loose_step
Step = collections.namedtuple("Step", "acc way pp filter")


def mont_point(pt):
    """affine canonical coordinates (ints, or pairs of ints for G2) -> the Montgomery limb tuples a kernel holds"""
    m = lambda c: limbs(c * RADIX_P % P, FP_NL)
    return tuple((m(c[0]), m(c[1])) if isinstance(c, tuple) else m(c) for c in pt)


def xyzz_inf(two):
    F = _F2 if two else _F1
    return tuple(F.to_limbs(c) for c in (F.one, F.one, F.zero, F.zero))


def xyzz_add_mixed_loose(p, q):
    """bls::xyzz_add_mixed_loose(p, q), p = (x, y, zz, zzz) loose limb tuples, q = mont_point(...). Returns Step: the sum, the way
    it went (WAYS), the difference pp_ the filter looked at and what lz_maybe_zero said per component. 'false_positive': the
    filter passed, the exact test (a canonicalisation) said non-zero, and the addition went on with the loose formulas; the exact
    formulas run only for a true doubling or cancellation."""
    two = _is2(q[0])
    B = BOUND[two]
    F = _F2 if two else _F1
    if lf_is_zero(p[2]):
        return Step((q[0], q[1], F.to_limbs(F.one), F.to_limbs(F.one)), "first", None, None)
    u2, s2 = lf_mul(q[0], p[2]), lf_mul(q[1], p[3])
    pp_ = lf_sub(B["X"], u2, p[0])
    filt = tuple(lz_maybe_zero(c) for c in components(pp_))
    if all(filt) and lf_is_zero(lf_canon(pp_)):
        acc, way = xyzz_add_mixed(tuple(lf_canon(c) for c in p), q)
        assert way != "general"
        return Step(acc, way, pp_, filt)
    rr = lf_sub(B["Y"], s2, p[1])
    pp = lf_sqr(B["M"] + B["X"], pp_)
    ppp, qq = lf_mul(pp_, pp), lf_mul(p[0], pp)
    x = lf_sub(3 * B["M"], lf_sqr(B["M"] + B["Y"], rr), lf_add_nc(ppp, lf_add_nc(qq, qq)))
    if B["WEAK"]:
        x = lf_weak(B["X"], x)
    y = lf_sub(B["M"], lf_mul(rr, lf_sub(B["X"], qq, x)), lf_mul(p[1], ppp))
    return Step((x, y, lf_mul(p[2], pp), lf_mul(p[3], ppp)), "false_positive" if all(filt) else "loose", pp_, filt)


def within_bounds(acc):
    """the accumulator respects LooseBound: normalised limbs, x < X p, y < Y p, zz and zzz < M p, per F_p component"""
    B = BOUND[_is2(acc[0])]
    for c, k in zip(acc, (B["X"], B["Y"], B["M"], B["M"])):
        for f in components(c):
            if max(f) > LM or value(f) >= k * P:
                return False
    return True


def chain(points):
    """the bucket accumulation of k_bucket_sum over affine canonical points: (final accumulator, [Step, ...])"""
    two = isinstance(points[0][0], tuple)
    acc, steps = xyzz_inf(two), []
    for pt in points:
        st = xyzz_add_mixed_loose(acc, mont_point(pt))
        steps.append(st)
        acc = st.acc
    return acc, steps


def pair_ways(a, b):
    """the way of the second addition of a two-point bucket, in both orders"""
    return chain([a, b])[1][1].way, chain([b, a])[1][1].way


# ---- curve points by x -----------------------------------------------------------------------------------------------------------
def sqrt_fp(a):
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def fp2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def sqrt_fp2(a):
    """a square root in F_p[u]/(u^2 + 1), p = 3 mod 4, or None"""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = sqrt_fp(a0)
        if s is not None:
            return (s, 0)
        s = sqrt_fp(-a0 % P)
        return (0, s)                       # (s u)^2 = -s^2; one of a0, -a0 is a square
    alpha = sqrt_fp((a0 * a0 + a1 * a1) % P)
    if alpha is None:
        return None
    inv2 = (P + 1) // 2
    for sign in (1, -1):
        x0 = sqrt_fp((a0 + sign * alpha) * inv2 % P)
        if x0:
            s = (x0, a1 * pow(2 * x0, -1, P) % P)
            if fp2_mul(s, s) == (a0, a1):
                return s
    return None


def g1_from_mont_x(X):
    """the point whose x coordinate has the Montgomery form X, or None (on the curve y^2 = x^3 + 4, not in the r-subgroup in general:
    the MSM does not ask for membership and the a = 0 formulas never use b)"""
    x = X * RP_INV % P
    y = sqrt_fp((x * x * x + 4) % P)
    return None if y is None else (x, y)


def g2_from_mont_x(X):
    x = (X[0] * RP_INV % P, X[1] * RP_INV % P)
    x3 = fp2_mul(fp2_mul(x, x), x)
    y = sqrt_fp2(((x3[0] + 4) % P, (x3[1] + 4) % P))
    return None if y is None else (x, y)


def g1_on_curve(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 - 4) % P == 0


def g2_on_curve(pt):
    x, y = pt
    x3, y2 = fp2_mul(fp2_mul(x, x), x), fp2_mul(y, y)
    return (y2[0] - x3[0] - 4) % P == 0 and (y2[1] - x3[1] - 4) % P == 0


def random_g1(rng):
    while True:
        pt = g1_from_mont_x(rand_below(rng, P))
        if pt:
            return pt


def random_g2(rng):
    while True:
        pt = g2_from_mont_x((rand_below(rng, P), rand_below(rng, P)))
        if pt:
            return pt


def mont_x(pt):
    x = pt[0]
    return (x[0] * RADIX_P % P, x[1] * RADIX_P % P) if isinstance(x, tuple) else x * RADIX_P % P


def alias(X, d, rng):
    """a Montgomery value below p that is X + d p in its low 28 bits and random above: against X as the first point of a bucket the
    filter sees (d or d + 1) p in the low limb of the difference"""
    low = (X + d * P) & LM
    while True:
        v = (rand_below(rng, P >> LB) << LB) | low
        if v < P and v != X:
            return v


D_WINDOW = 7    # |d| <= 7 keeps d, d + 1 and their negatives inside the filter's [-8, 23] (G1) and [-16, 15] (G2) in both orders


def g1_alias_of(X, rng, dmin=-D_WINDOW, dmax=D_WINDOW):
    while True:
        pt = g1_from_mont_x(alias(X, dmin + rand_below(rng, dmax - dmin + 1), rng))
        if pt:
            return pt


def g2_alias_of(X, rng, mode="both", dmin=-D_WINDOW, dmax=D_WINDOW):
    """mode 'both': both components aliased; 'c0_zero': c0 EQUAL (a zero-residue component inside the loose general formulas), c1
    random; 'c0_alias_c1_equal': c0 aliased, c1 equal"""
    d = lambda: dmin + rand_below(rng, dmax - dmin + 1)
    while True:
        if mode == "both":
            Xn = (alias(X[0], d(), rng), alias(X[1], d(), rng))
        elif mode == "c0_zero":
            Xn = (X[0], rand_below(rng, P))
        else:
            Xn = (alias(X[0], d(), rng), X[1])
        pt = g2_from_mont_x(Xn)
        if pt and Xn != X:
            return pt


def g1_false_positive_pair(rng):
    a = random_g1(rng)
    return a, g1_alias_of(mont_x(a), rng)


def g2_false_positive_pair(rng, mode="both"):
    a = random_g2(rng)
    return a, g2_alias_of(mont_x(a), rng, mode)


def g1_family(rng, count):
    """count distinct points, any two of them a false positive in either order: every x is base + d p in the low limb, d in 0..7"""
    base = rand_below(rng, P)
    out, seen = [], set()
    while len(out) < count:
        pt = g1_alias_of(base, rng, 0, D_WINDOW)
        if pt[0] not in seen:
            seen.add(pt[0])
            out.append(pt)
    return out


def g2_family(rng, count):
    base = (rand_below(rng, P), rand_below(rng, P))
    out, seen = [], set()
    while len(out) < count:
        pt = g2_alias_of(base, rng, "both", 0, D_WINDOW)
        if pt[0] not in seen:
            seen.add(pt[0])
            out.append(pt)
    return out


SAT = (1 << (LB * (FP_NL - 1))) - 1      # thirteen limbs of ones


def g1_saturated(count, start=0):
    """points whose Montgomery x is thirteen saturated limbs under a top limb below p's: the columns of the product scan at their
    largest"""
    out, top = [], start
    while len(out) < count:
        pt = g1_from_mont_x((top << (LB * (FP_NL - 1))) | SAT)
        top += 1
        assert top < P >> (LB * (FP_NL - 1))
        if pt:
            out.append(pt)
    return out


def g2_saturated(count, start=0):
    out, top = [], start
    while len(out) < count:
        pt = g2_from_mont_x(((top << (LB * (FP_NL - 1))) | SAT, ((top + 1000) << (LB * (FP_NL - 1))) | SAT))
        top += 1
        if pt:
            out.append(pt)
    return out


def is_saturated(pt):
    return all(limbs(X, FP_NL)[:FP_NL - 1] == (LM,) * (FP_NL - 1) for X in (mont_x(pt) if isinstance(pt[0], tuple) else [mont_x(pt)]))


# ---- a false positive against a LOOSE accumulator (fixed order: the CPU only) ---------------------------------------------------
def loose_false_positive(prefix, rng, max_tries=400):
    """a point q such that adding it to the accumulator of `prefix` (two or more points: zz != 1, coordinates unreduced) passes the
    filter with a non-zero difference. u2 = lz_mul(x3 R, zz) is x3 R zz / R mod p plus a small multiple j p (j <= 1 for G1; for G2
    the Karatsuba recombination adds up to 2 + 4 p per component): pick the residue T with the low limb of acc.x + (k - X) p for a
    k in the middle of the filter's 32, solve x3 = T R / zz, keep it when it is on the curve."""
    acc, _ = chain(prefix)
    two = _is2(acc[0])
    B = BOUND[two]
    want = lambda xc: (value(xc) + (12 - B["X"]) * P) & LM
    for _ in range(max_tries):
        if two:
            T = tuple((rand_below(rng, P >> LB) << LB) | want(acc[0][i]) for i in range(2))
            if max(T) >= P:
                continue
            zz = (value(acc[2][0]) % P, value(acc[2][1]) % P)      # Montgomery zz; x3 R = T R / zz in F_p^2
            n = pow(zz[0] * zz[0] + zz[1] * zz[1], -1, P)
            zi = (zz[0] * n % P, -zz[1] * n % P)
            X3 = fp2_mul(fp2_mul(T, zi), (RADIX_P % P, 0))
            q = g2_from_mont_x(X3)
        else:
            T = (rand_below(rng, P >> LB) << LB) | want(acc[0])
            if T >= P:
                continue
            q = g1_from_mont_x(T * RADIX_P % P * pow(value(acc[2]), -1, P) % P)
        if q and xyzz_add_mixed_loose(acc, mont_point(q)).way == "false_positive":
            return q
    return None


# ---- API forms -----------------------------------------------------------------------------------------------------------------
def u64x(v, n):
    return [(int(v) >> (64 * i)) & M64 for i in range(n)]


def fr_rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def fr_ints(a):
    buf = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def fr_random(rng, n):
    """n uniform values below r, the ones in [2^254, r) included"""
    buf = rng.bytes(32 * n)
    m = (1 << 255) - 1
    vals = (int.from_bytes(buf[i:i + 32], "little") & m for i in range(0, len(buf), 32))
    return [v - R if v >= R else v for v in vals]


def g1_rows(pts):
    return np.array([u64x(p[0], 6) + u64x(p[1], 6) for p in pts], dtype=np.uint64).reshape(-1, 12)


def g2_rows(pts):
    return np.array([u64x(p[0][0], 6) + u64x(p[0][1], 6) + u64x(p[1][0], 6) + u64x(p[1][1], 6) for p in pts], dtype=np.uint64).reshape(-1, 24)


def scalar_rows(ks):
    return np.array([u64x(k, 4) for k in ks], dtype=np.uint64).reshape(-1, 4)


Case = collections.namedtuple("Case", "inputs witnesses planted wanted")
"""inputs: what the GPU test feeds; witnesses: the operand pairs (or point pairs) that take the planted path; planted / wanted: the
positions that got a constructed element / that the pattern asked for (a construction may fail: the rest is random data)"""


def fill_share(case):
    return 1.0 if not case.wanted else case.planted / case.wanted


# ---- R1CS cases (systems in the form of tests/r1cs_cases.py) ------------------------------------------------------------------
LONG_ROW_THRESHOLD = 128
R1CS_ROWS = 1280               # five workgroups of k_eval_short / k_check, 768 padding rows


def _csr(rows):
    """rows: list of [(wire, coefficient index), ...]"""
    ptr, col, cf = [0], [], []
    for row in rows:
        for w, k in row:
            col.append(w)
            cf.append(k)
        ptr.append(len(col))
    return np.array(ptr, np.uint64), np.array(col, np.uint32), np.array(cf, np.uint32)


def r1cs_general_case(pattern, seed, long_terms=(700, 300)):
    """Unsatisfied system for evaluation parity and the fused check. Matrix A: every row has an addition and two general terms, the
    first general term planted (fr_mul(coeff R, w) subtracts) where the pattern says so; row 7 has long_terms[0] general terms,
    planted by the same pattern over its terms (k_eval_long: term t is lane t mod 256). Matrix B: a small and a negative-small
    term per row, from the one-subtraction pairs of mul_small where the pattern says so, remainder-just-below-r pairs elsewhere;
    row 300 has long_terms[1] small terms. Matrix C: a general and a subtraction term. Two coefficients of the table are ones
    whose conversion at create subtracts."""
    rng = np.random.default_rng(seed)
    n = R1CS_ROWS
    mask = patterns(n)[pattern]
    coeffs = [1, R - 1] + [rand_below(rng, R - (1 << 200)) + (1 << 100) for _ in range(6)]
    load = [plant_fr_load(rng) for _ in range(2)]
    wit_create = [(c, R2_R) for c in load if c is not None]
    coeffs += [c if c is not None else rand_below(rng, R) for c in load]
    GEN = list(range(2, len(coeffs)))
    index = {c: i for i, c in enumerate(coeffs)}

    def coeff_id(c):
        if c not in index:
            index[c] = len(coeffs)
            coeffs.append(c)
        return index[c]

    w = [1]
    wit_short, wit_long, wit_small = [], [], []
    planted = wanted = 0

    def general_term(plant, sink):
        nonlocal planted, wanted
        k = GEN[rand_below(rng, len(GEN))]
        b = fr_mont(coeffs[k])
        v = None
        if plant:
            wanted += 1
            v = plant_fr(b, rng)
            if v is not None:
                planted += 1
                sink.append((b, v))
        w.append(rand_below(rng, R) if v is None else v)
        return (len(w) - 1, k)

    one_sub, near = mul_small_pairs(rng, 2 * n + long_terms[1])
    A, Bm, C = [], [], []
    for j in range(n):
        if j == 7:
            lm = patterns(long_terms[0])[pattern]
            A.append([general_term(bool(lm[t]), wit_long) for t in range(long_terms[0])])
        else:
            A.append([(0, 0), general_term(bool(mask[j]), wit_short), general_term(False, wit_short)])
        row = []
        for neg in ((False,) * long_terms[1] if j == 300 else (False, True)):
            ww, c = (one_sub if mask[j] or j == 300 else near).pop()
            if mask[j] or j == 300:
                wit_small.append((ww, c))
            w.append(ww)
            row.append((len(w) - 1, coeff_id(R - c if neg else c)))
        Bm.append(row)
        C.append([general_term(False, wit_short), (1 + rand_below(rng, len(w) - 1), 1)])
    s = {"n": n, "n_wires": len(w), "coeffs": coeffs, "mats": [_csr(A), _csr(Bm), _csr(C)], "w": w}
    wit = {"short": wit_short, "long": wit_long, "create": wit_create, "small": wit_small}
    return Case(s, wit, planted + len(wit_create), wanted + 2)


def r1cs_product_case(pattern, seed):
    """Satisfied system for the check: A_j = w_x, B_j = w_y, C_j = w_z = w_x w_y, with fr_mul(w_x, w_y) subtracting inside k_check
    where the pattern says so. inputs = (system, the rows to break: w_z + 1 there must be counted)"""
    rng = np.random.default_rng(seed)
    n = R1CS_ROWS
    mask = patterns(n)[pattern]
    w, wit, planted = [1], [], 0
    A, Bm, C = [], [], []
    for j in range(n):
        y = rand_below(rng, R - 1) + 1
        x = plant_fr(y, rng) if mask[j] else None
        if x is not None:
            planted += 1
            wit.append((x, y))
        else:
            x = rand_below(rng, R)
        base = len(w)
        w += [x, y, x * y % R]
        A.append([(base, 0)]); Bm.append([(base + 1, 0)]); C.append([(base + 2, 0)])
    s = {"n": n, "n_wires": len(w), "coeffs": [1], "mats": [_csr(A), _csr(Bm), _csr(C)], "w": w}
    planted_rows = [j for j in range(n) if mask[j]]
    broken = sorted({planted_rows[len(planted_rows) // 3], planted_rows[-1], n - 1, 70})
    return Case((s, broken), wit, planted, int(mask.sum()))


# ---- F_r NTT cases ---------------------------------------------------------------------------------------------------------------
LOG_TILE = 10
NTT_SITES = ("load", "coset_scale", "first_stage", "second_kernel", "third_kernel", "store_coset")
COSET_SHIFT = 7
COSET_INV = pow(COSET_SHIFT, -1, R)


def powers(base, n):
    out, v = [], 1
    for _ in range(n):
        out.append(v)
        v = v * base % R
    return out


def ntt_plan(log_n):
    """the stages each kernel of fr_ntt_run does: [(kernel, stages done before it)], as the host code splits them"""
    tile = min(log_n, LOG_TILE)
    top = log_n - tile
    passes = (top + 6) // 7
    out, done = [], 0
    for k in range(passes):
        out.append(("colpass<%s>" % ("true" if k == 0 else "false"), done))
        done += top // passes + (1 if k < top % passes else 0)
    out.append(("tile<%s,true>" % ("false" if passes else "true"), done))
    return out


def root(log_n, inverse=False):
    w = pow(7, (R - 1) >> log_n, R)
    return pow(w, -1, R) if inverse else w


def dif_stages(x, log_n, s, inverse=False):
    """the array after the first s decimation-in-frequency stages of the transform (plain values)"""
    n, w = 1 << log_n, root(log_n, inverse)
    x = list(x)
    for st in range(s):
        L = n >> st
        h = L // 2
        tw = [pow(w, i << st, R) for i in range(h)]
        for blk in range(0, n, L):
            for i in range(h):
                u, v = x[blk + i], x[blk + i + h]
                x[blk + i], x[blk + i + h] = (u + v) % R, (u - v) * tw[i] % R
    return x


def after_stages_at(x, log_n, s, pos, inverse=False):
    """element `pos` of dif_stages(x, log_n, s) from the 2^s inputs of its stride class alone"""
    n, L = 1 << log_n, (1 << log_n) >> s
    blk, i = pos // L, pos % L
    c = int(format(blk, "0%db" % s)[::-1], 2) if s else 0
    w = root(log_n, inverse)
    return pow(w, i * c, R) * sum(x[i + t * L] * pow(w, (t * L * c) % n, R) for t in range(1 << s)) % R


def _bitrev(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2) if bits else 0


def inputs_for_intermediate(y, log_n, s, fr_ntt, inverse=False):
    """the transform input (rows) whose array after s stages is y (plain values): finish the transform of every block of y with
    `fr_ntt` (the oracle's), put the outputs where the full transform has them, and transform back. A transform with omega^-1 is
    the forward one read backwards."""
    n, L = 1 << log_n, (1 << log_n) >> s
    back = lambda rows: np.concatenate([rows[:1], rows[:0:-1]])
    Y = fr_rows(y)
    X = np.zeros((n, 4), np.uint64)
    for blk in range(1 << s):
        sub = Y[blk * L:(blk + 1) * L]
        if L > 1:
            sub = fr_ntt(sub, inverse=False)
            if inverse:
                sub = back(sub)
        X[_bitrev(blk, s)::1 << s] = sub
    x = fr_ntt(X, inverse=True)          # x_j = 1/n sum X_k w^-jk; the inverse transform wants 1/n sum X_k w^+jk
    return back(x) if inverse else x


def ntt_case(log_n, site, pattern, seed, fr_ntt):
    """One transform whose `site` multiplication subtracts where the pattern says so. inputs = dict(values, inverse, shift);
    fr_ntt: the oracle's transform (the module itself stays free of the oracle). The pattern runs over the elements in natural
    order (for a butterfly site: over the lower elements of the pairs, which is the order of the lanes)."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    plan = ntt_plan(log_n)
    wit, planted = [], 0
    if site in ("load", "coset_scale"):
        mask = patterns(n)[pattern]
        shift = COSET_SHIFT if site == "coset_scale" else None
        x = fr_random(rng, n)
        for i in np.nonzero(mask)[0].tolist():
            if site == "load":
                v = plant_fr_load(rng)
                w = (v, R2_R)
            else:
                b = fr_mont(pow(COSET_SHIFT, i, R))
                a = plant_fr(b, rng)
                v, w = (None, None) if a is None else (a * RR_INV % R, (a, b))
            if v is not None:
                x[i], planted = v, planted + 1
                wit.append(w)
        return Case(dict(values=fr_rows(x), inverse=False, shift=shift), wit, planted, int(mask.sum()))
    if site in ("first_stage", "second_kernel", "third_kernel"):
        k = NTT_SITES.index(site) - 2
        if k >= len(plan):
            return None
        s = plan[k][1]
        inverse = seed % 2 == 1 and s > 0          # the inverse transform shares the butterflies: odd seeds run it
        L = n >> s
        h = L // 2
        w = root(log_n, inverse)
        y = fr_random(rng, n)
        lows = [blk + i for blk in range(0, n, L) for i in range(h)]
        mask = patterns(len(lows))[pattern]
        for t in np.nonzero(mask)[0].tolist():
            lo = lows[t]
            b = fr_mont(pow(w, (lo % L) << s, R))
            d = plant_fr(b, rng)
            if d is None:
                continue
            y[lo] = (y[lo + h] + d * RR_INV) % R
            planted += 1
            wit.append((d, b))
        x = fr_rows(y) if s == 0 else inputs_for_intermediate(y, log_n, s, fr_ntt, inverse)
        return Case(dict(values=x, inverse=inverse, shift=None, stages_before=s, intermediate=y), wit, planted, int(mask.sum()))
    # the store of the inverse coset transform: choose the output, get the input from the forward transform. The scaled value V'
    # (Montgomery form of output * shift^i) subtracts against the coset power shift^-i. (The 1/n scale before it admits no
    # operand: tests/test_bls_rare_paths.py::test_constants_that_admit_no_operand.)
    assert site == "store_coset"
    mask = patterns(n)[pattern]
    out = fr_random(rng, n)
    for i in np.nonzero(mask)[0].tolist():
        power = pow(COSET_INV, i, R)
        b = fr_mont(power)
        a = plant_fr(b, rng)
        if a is not None:
            out[i], planted = a * RR_INV % R * power % R, planted + 1
            wit.append((a, b))
    x = fr_ntt(fr_rows(out), inverse=False, shift=COSET_SHIFT)
    return Case(dict(values=x, inverse=True, shift=COSET_SHIFT, output=out), wit, planted, int(mask.sum()))


# ---- Groth16 quotient ------------------------------------------------------------------------------------------------------------
def quotient_case(log_n, pattern, seed, fr_ntt):
    """a, b, c whose coset evaluations make both products of k_quotient_pointwise subtract: A B with A = plant(B), and
    (A B - C) den with A B - C = plant(den)"""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    mask = patterns(n)[pattern]
    den = fr_mont(pow(pow(COSET_SHIFT, n, R) - 1, -1, R))
    ca, cb, cc, wit, planted = [], [], [], [], 0
    for i in range(n):
        b = rand_below(rng, R - 1) + 1
        a = c = None
        if mask[i]:
            A, D = plant_fr(fr_mont(b), rng), plant_fr(den, rng)
            if A is not None and D is not None:
                a = A * RR_INV % R
                c = (a * b - D * RR_INV) % R
                wit += [(A, fr_mont(b)), (D, den)]
                planted += 1
        if a is None:
            a, c = rand_below(rng, R), rand_below(rng, R)
        ca.append(a); cb.append(b); cc.append(c)
    back = lambda ev: fr_ntt(fr_ntt(fr_rows(ev), inverse=True, shift=COSET_SHIFT), inverse=False)
    return Case(dict(a=back(ca), b=back(cb), c=back(cc), coset=(ca, cb, cc)), wit, planted, int(mask.sum()))


# ---- MSM cases -------------------------------------------------------------------------------------------------------------------
MSM_C = 5                      # the window width of every point count below 1024
HEAVY, HEAVY_CHUNK = 128, 8192


def msm_heavy_limit(n, c=MSM_C):
    """a bucket of more points than this is summed by k_heavy_sum (msm.inc: HEAVY << hs)"""
    hs = 0
    while (HEAVY << hs) < 4 * (n >> (c - 1)):
        hs += 1
    return HEAVY << hs


def _bucket_scalar(slot):
    """the scalar that puts a point into bucket `slot` and no other: digit 1 + slot % 16 of window slot // 16"""
    return (1 + slot % 16) << (MSM_C * (slot // 16))


def msm_pairs_case(group, layout, seed, mode="both"):
    """Two-point buckets. layout 'one': a single bucket; 'wave': 64 buckets (with every other bucket empty they are the first wave of
    k_bucket_sum); 'alternate': 128 two-point buckets, every other one a false-positive pair, the rest random pairs.
    inputs = (scalars, points as ints); witnesses: the pairs."""
    rng = np.random.default_rng(seed)
    fp = (lambda: g1_false_positive_pair(rng)) if group == 1 else (lambda: g2_false_positive_pair(rng, mode))
    rnd = (lambda: (random_g1(rng), random_g1(rng))) if group == 1 else (lambda: (random_g2(rng), random_g2(rng)))
    slots = {"one": 1, "wave": 64, "alternate": 128}[layout]
    pts, ks, wit = [], [], []
    for s in range(slots):
        special = layout != "alternate" or s % 2 == 0
        pair = fp() if special else rnd()
        if special:
            wit.append(pair)
        pts += list(pair)
        ks += [_bucket_scalar(s)] * 2
    order = rng.permutation(len(pts)).tolist()
    return Case(([ks[i] for i in order], [pts[i] for i in order]), wit, len(wit), len(wit))


def msm_heavy_case(group, seed, count=None):
    """one heavy bucket of pairwise false-positive points: the first addition of every lane of k_heavy_sum is one, whatever order
    the sort left them in. A few other points in other buckets."""
    rng = np.random.default_rng(seed)
    count = count or (600 if group == 1 else 300)
    fam = g1_family(rng, count) if group == 1 else g2_family(rng, count)
    extra = [random_g1(rng) if group == 1 else random_g2(rng) for _ in range(8)]
    ks = [1] * count + [rand_below(rng, 1 << 256) for _ in extra]
    assert count > msm_heavy_limit(count + len(extra))
    return Case((ks, fam + extra), fam, count, count)


def msm_saturated_case(group, seed, generator_multiples):
    """saturated-limb points in ordinary buckets (random full scalars, and pairs of them sharing a bucket) and in one heavy
    bucket, mixed with the given multiples of the generator"""
    rng = np.random.default_rng(seed)
    n_heavy = 560 if group == 1 else 280
    sat = g1_saturated(n_heavy + 40) if group == 1 else g2_saturated(n_heavy + 40)
    gens = list(generator_multiples)
    pts = sat[:n_heavy] + gens[:8]
    ks = [3] * (n_heavy + 8)                                   # the heavy bucket: digit 3 of window 0
    for i, q in enumerate(sat[n_heavy:]):                      # two saturated points per bucket, then full scalars
        pts.append(q)
        ks.append(_bucket_scalar(40 + i // 2) if i < 20 else rand_below(rng, 1 << 256))
    for q in gens[8:]:
        pts.append(q)
        ks.append(rand_below(rng, 1 << 256))
    assert n_heavy + 8 > msm_heavy_limit(len(pts))
    return Case((ks, pts), sat, len(sat), len(sat))
