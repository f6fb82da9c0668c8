"""An independent BLS12-381 pairing in Python integers, the reference of the pairing tests. Deliberately unlike the kernels
(city-rollup_amd/csrc/pairing.h): affine coordinates, slopes taken in F_p^2 on the twist (where an inversion is cheap) and the
unscaled line mapped into F_p^12, dense F_p^12 multiplication, no sparse lines, no cyclotomic squaring, no Frobenius map, and
the final exponent as ONE integer power c (p^12 - 1) / r, with the library's c as a parameter.

F_p^12 = F_p^2[w] / (w^6 - xi), xi = 1 + u, F_p^2 = F_p[u] / (u^2 + 1). An element is a list of six (c0, c1) pairs, the
coefficients of w^0 .. w^5: the coefficient order of the library's GT values (include/cityprover.h), so gt_to_words /
gt_from_words are plain splitting into 64-bit words."""
X_ABS = 0xd201000000010000
R = X_ABS**4 - X_ABS**2 + 1
P = (X_ABS + 1)**2 * R // 3 - X_ABS
assert P == 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
G1 = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
      0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
G2 = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
       0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
      (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
       0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))


# ---- F_p^2 ----
def f2_add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def f2_sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
def f2_scale(a, s): return (a[0] * s % P, a[1] * s % P)
def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * d % P, -a[1] * d % P)


XI = (1, 1)
XI_INV = f2_inv(XI)
F12_ONE = [(1, 0)] + [(0, 0)] * 5
F12_ZERO = [(0, 0)] * 6


# ---- F_p^12, dense: the 11 coefficients of the polynomial product unreduced, then w^6 = xi and one reduction mod p ----
def f12_mul(a, b):
    re, im = [0] * 11, [0] * 11
    for i in range(6):
        a0, a1 = a[i]
        if a0 == 0 and a1 == 0:
            continue
        for j in range(6):
            b0, b1 = b[j]
            re[i + j] += a0 * b0 - a1 * b1
            im[i + j] += a0 * b1 + a1 * b0
    out = []
    for k in range(6):
        r, m = re[k], im[k]
        if k < 5:  # (hr + hm u)(1 + u)
            r, m = r + re[k + 6] - im[k + 6], m + re[k + 6] + im[k + 6]
        out.append((r % P, m % P))
    return out


def f12_pow(a, e):
    assert e >= 0
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_inv(a):
    return f12_pow(a, P**12 - 2)


# ---- the curve and the twist, affine; None is infinity ----
def g1_on_curve(p): return (p[1] * p[1] - p[0]**3 - 4) % P == 0
def g2_on_curve(q): return f2_sub(f2_mul(q[1], q[1]), f2_add(f2_mul(f2_mul(q[0], q[0]), q[0]), (4, 4))) == (0, 0)


def _line(t, slope, p):
    """the line through the untwisted image of t (a twist point) with twist slope `slope`, at p in G1, as an element of F_p^12.
    Untwist: (x', y') -> (x' / w^2, y' / w^3); 1 / w = w^5 / xi and 1 / w^3 = w^3 / xi. The slope of the images is slope / w:
        l = yp - (slope xp / xi) w^5 + ((slope x'_t - y'_t) / xi) w^3"""
    c5 = f2_mul(f2_scale(slope, -p[0] % P), XI_INV)
    c3 = f2_mul(f2_sub(f2_mul(slope, t[0]), t[1]), XI_INV)
    return [(p[1] % P, 0), (0, 0), (0, 0), c3, (0, 0), c5]


def _vertical(t, p):
    """x - x_t for the untwisted t: xp - x'_t w^4 / xi"""
    return [(p[0] % P, 0), (0, 0), (0, 0), (0, 0), f2_sub((0, 0), f2_mul(t[0], XI_INV)), (0, 0)]


def twist_double(t):
    s = f2_mul(f2_scale(f2_mul(t[0], t[0]), 3), f2_inv(f2_scale(t[1], 2)))
    x3 = f2_sub(f2_mul(s, s), f2_scale(t[0], 2))
    return (x3, f2_sub(f2_mul(s, f2_sub(t[0], x3)), t[1])), s


def twist_add(t, q):
    s = f2_mul(f2_sub(q[1], t[1]), f2_inv(f2_sub(q[0], t[0])))
    x3 = f2_sub(f2_sub(f2_mul(s, s), t[0]), q[0])
    return (x3, f2_sub(f2_mul(s, f2_sub(t[0], x3)), t[1])), s


def miller_loop(p, q):
    """f_{|x|, Q}(P) with the lines as they are (no scaling), inverted at the end for the sign of x by the conjugate w -> -w,
    which is the inverse up to a factor the final exponentiation removes"""
    f, t = F12_ONE, q
    for bit in bin(X_ABS)[3:]:
        t2, s = twist_double(t)
        f = f12_mul(f12_mul(f, f), _line(t, s, p))
        t = t2
        if bit == "1":
            t2, s = twist_add(t, q)
            f = f12_mul(f, _line(t, s, p))
            t = t2
    return [c if k % 2 == 0 else f2_sub((0, 0), c) for k, c in enumerate(f)]


def final_exponent(c):
    assert (P**12 - 1) % R == 0
    return c * ((P**12 - 1) // R)


def pairing(p, q, c=1):
    """e(P, Q)^c; None for either point gives one"""
    if p is None or q is None:
        return F12_ONE
    assert g1_on_curve(p) and g2_on_curve(q)
    return f12_pow(miller_loop(p, q), final_exponent(c))


_cache = {}


def e_generators(c):
    """e(G1, G2)^c, computed once per process"""
    if c not in _cache:
        _cache[c] = pairing(G1, G2, c)
    return _cache[c]


def gt_power(c, k):
    """e(G1, G2)^(c k): the expected value of any product of pairings of known multiples of the generators"""
    return f12_pow(e_generators(c), k % R)


# ---- the library's GT layout: 12 coefficients x 6 little-endian u64 ----
def gt_to_words(a):
    return [(v >> (64 * i)) & (2**64 - 1) for c in a for v in c for i in range(6)]


def gt_from_words(w):
    vals = [sum(int(w[6 * j + i]) << (64 * i) for i in range(6)) for j in range(12)]
    return [(vals[2 * k], vals[2 * k + 1]) for k in range(6)]
