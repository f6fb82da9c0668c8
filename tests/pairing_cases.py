"""Inputs shared by the pairing tests (tests/test_pairing_host.py, tests/test_gpu_pairing.py, tests/test_gpu_groth16_verify.py):
word conversions, multiples of the generators by the oracle, and points ON the curve / twist but OUTSIDE the r-torsion (a small
x and a square root in Python integers; p = 3 mod 4). Nothing here touches the GPU or the library."""
import numpy as np

import oracle_lib as O
import pairing_ref as PR

P, R = PR.P, PR.R
MASK = 2**64 - 1


def w6(v):
    return [(v >> (64 * i)) & MASK for i in range(6)]


def g1_words(pt):
    """(x, y) -> 12 u64; None -> zeros"""
    return np.zeros(12, np.uint64) if pt is None else np.array(w6(pt[0]) + w6(pt[1]), np.uint64)


def g2_words(pt):
    if pt is None:
        return np.zeros(24, np.uint64)
    (x0, x1), (y0, y1) = pt
    return np.array(w6(x0) + w6(x1) + w6(y0) + w6(y1), np.uint64)


def f2_words(a):
    return np.array(w6(a[0]) + w6(a[1]), np.uint64)


def f2_from_words(w):
    val = lambda a: sum(int(v) << (64 * j) for j, v in enumerate(a))
    return (val(w[0:6]), val(w[6:12]))


def gt_words(a):
    return np.array(PR.gt_to_words(a), np.uint64)


def g1_mul(k):
    return O.bls_g1_mul(PR.G1, k % R)


def g2_mul(k):
    return O.bls_g2_mul(PR.G2, k % R)


def g1_neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def g2_neg(pt):
    return None if pt is None else (pt[0], PR.f2_sub((0, 0), pt[1]))


# ---- square roots (the recipe of tests/test_groth16_pack.py) ----
def fp_sqrt(a):
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def f2_pow(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = PR.f2_mul(out, a)
        a = PR.f2_mul(a, a)
        e >>= 1
    return out


def f2_sqrt(a):
    if a == (0, 0):
        return a
    a1 = f2_pow(a, (P - 3) // 4)
    alpha, x0 = PR.f2_mul(PR.f2_mul(a1, a1), a), PR.f2_mul(a1, a)
    y = PR.f2_mul((0, 1), x0) if alpha == (P - 1, 0) else PR.f2_mul(f2_pow(PR.f2_add((1, 0), alpha), (P - 1) // 2), x0)
    return y if PR.f2_mul(y, y) == a else None


_outside = {}


def g1_outside_torsion():
    """a point of E(F_p) with [r] P != infinity (asserted by the oracle): the first small x with a square right-hand side"""
    if "g1" not in _outside:
        for x in range(1, 200):
            y = fp_sqrt((x**3 + 4) % P)
            if y is not None and O.bls_g1_mul((x, y), R) is not None:
                _outside["g1"] = (x, y)
                break
    pt = _outside["g1"]
    assert PR.g1_on_curve(pt) and O.bls_g1_on_curve(pt) and O.bls_g1_mul(pt, R) is not None
    return pt


def g2_outside_torsion():
    if "g2" not in _outside:
        for x in range(1, 200):
            xx = (x, 0)
            y = f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(xx, xx), xx), (4, 4)))
            if y is not None and O.bls_g2_mul((xx, y), R) is not None:
                _outside["g2"] = (xx, y)
                break
    pt = _outside["g2"]
    assert PR.g2_on_curve(pt) and O.bls_g2_on_curve(pt) and O.bls_g2_mul(pt, R) is not None
    return pt


def scalars(n, seed):
    """n distinct non-zero scalars below r: the small ones first (1, 2, 3, r - 1, 2^64, ...), then full-width random ones"""
    rng = np.random.default_rng(seed)
    out = [1, 2, 3, R - 1, 1 << 64, (1 << 128) + 5, R - 2, 7]
    while len(out) < n:
        k = int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1
        if k not in out:
            out.append(k)
    return out[:n]
