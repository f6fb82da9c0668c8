"""The pairing arithmetic of city-rollup_amd/csrc/pairing.h on the CPU (tests/pairingsim: the __host__ __device__ code the
kernels run, built for the host) against Python integers (tests/pairing_ref.py, which shares no formula with it), and the
reference's own sanity. No GPU."""
import ctypes

import numpy as np
import pytest

import pairing_cases as PC
import pairing_ref as PR

P, R = PR.P, PR.R
u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def ps():
    import simlibs
    return ctypes.CDLL(simlibs.build("pairingsim"))


def ptr(a):
    return a.ctypes.data_as(u64p)


def call12(fn, *args):
    """fn(inputs..., out): F_p^12 inputs as lists of pairs, ints passed through; returns the F_p^12 output"""
    out = np.zeros(72, np.uint64)
    keep = [PC.gt_words(a) if isinstance(a, list) else a for a in args]   # the arrays live until the call returns
    fn(*[ptr(a) if isinstance(a, np.ndarray) else a for a in keep], ptr(out))
    return PR.gt_from_words(out)


def rand12(rng):
    return [(int.from_bytes(rng.bytes(48), "little") % P, int.from_bytes(rng.bytes(48), "little") % P) for _ in range(6)]


EDGES = [PR.F12_ZERO, PR.F12_ONE, [(P - 1, P - 1)] * 6]


def operands(seed, n=4):
    rng = np.random.default_rng(seed)
    return EDGES + [rand12(rng) for _ in range(n)]


def conj(a):
    return [c if k % 2 == 0 else PR.f2_sub((0, 0), c) for k, c in enumerate(a)]


# ---- the reference's own sanity ----
def test_reference_pairing_is_non_degenerate_of_order_r_and_bilinear():
    e = PR.e_generators(1)
    assert e != PR.F12_ONE
    assert PR.f12_pow(e, R) == PR.F12_ONE
    assert PR.pairing(PC.g1_mul(5), PR.G2) == PR.f12_pow(e, 5)
    assert PR.gt_from_words(PR.gt_to_words(e)) == e
    assert PR.e_generators(3) == PR.f12_pow(e, 3)


# ---- the tower ----
def test_f12_mul_and_sqr(ps):
    ops = operands(1)
    for a in ops:
        assert call12(ps.ps_f12_sqr, a) == PR.f12_mul(a, a)
        for b in ops:
            assert call12(ps.ps_f12_mul, a, b) == PR.f12_mul(a, b)


def test_f12_inverse_and_conjugate(ps):
    for a in operands(2):
        inv = call12(ps.ps_f12_inv, a)
        if a == PR.F12_ZERO:
            assert inv == PR.F12_ZERO
        else:
            assert PR.f12_mul(inv, a) == PR.F12_ONE
        assert call12(ps.ps_f12_conj, a) == conj(a)
    a = operands(2)[-1]
    assert conj(a) == PR.f12_pow(a, P**6)     # the conjugate is the Frobenius map to the sixth


@pytest.mark.parametrize("j", [1, 2, 3])
def test_f12_frobenius(ps, j):
    for a in operands(3 + j, n=2):
        assert call12(ps.ps_f12_frobenius, a, j) == PR.f12_pow(a, P**j)


def test_frobenius_powers_compose_to_every_power(ps):
    """p^4 .. p^11 as compositions of the three maps and the conjugate (p^6): each against the integer power"""
    a = operands(9, n=1)[-1]
    f = lambda x, j: call12(ps.ps_f12_frobenius, x, j)
    c = lambda x: call12(ps.ps_f12_conj, x)
    routes = {4: lambda x: f(f(x, 2), 2), 5: lambda x: f(f(x, 3), 2), 6: c, 7: lambda x: c(f(x, 1)), 8: lambda x: c(f(x, 2)),
              9: lambda x: c(f(x, 3)), 10: lambda x: c(f(f(x, 2), 2)), 11: lambda x: c(f(f(x, 3), 2))}
    for j, route in routes.items():
        assert route(a) == PR.f12_pow(a, P**j), j


def embed6(c):
    return [c[0], (0, 0), c[1], (0, 0), c[2], (0, 0)]


def call6(fn, *args):
    out = np.zeros(36, np.uint64)
    keep = [np.concatenate([PC.f2_words(c) for c in a]) for a in args]
    fn(*[ptr(k) for k in keep], ptr(out))
    return [PC.f2_from_words(out[12 * i:12 * i + 12]) for i in range(3)]


def test_f6_mul_sqr_inverse(ps):
    rng = np.random.default_rng(6)
    r2 = lambda: (int.from_bytes(rng.bytes(48), "little") % P, int.from_bytes(rng.bytes(48), "little") % P)
    ops = [[(0, 0)] * 3, [(1, 0), (0, 0), (0, 0)], [(P - 1, P - 1)] * 3] + [[r2(), r2(), r2()] for _ in range(4)]
    for a in ops:
        assert embed6(call6(ps.ps_f6_sqr, a)) == PR.f12_mul(embed6(a), embed6(a))
        for b in ops:
            assert embed6(call6(ps.ps_f6_mul, a, b)) == PR.f12_mul(embed6(a), embed6(b))
        inv = call6(ps.ps_f6_inv, a)
        if a == ops[0]:
            assert inv == ops[0]
        else:
            assert PR.f12_mul(embed6(inv), embed6(a)) == PR.F12_ONE


def test_sparse_multiplication_is_the_dense_one(ps):
    rng = np.random.default_rng(7)
    r2 = lambda: (int.from_bytes(rng.bytes(48), "little") % P, int.from_bytes(rng.bytes(48), "little") % P)
    lines = [((0, 0), (0, 0), (0, 0)), ((P - 1, P - 1),) * 3] + [(r2(), r2(), r2()) for _ in range(4)]
    for a in operands(8):
        for l0, l2, l3 in lines:
            dense = [l0, (0, 0), l2, l3, (0, 0), (0, 0)]
            out = np.zeros(72, np.uint64)
            wa, w0, w2, w3 = PC.gt_words(a), PC.f2_words(l0), PC.f2_words(l2), PC.f2_words(l3)
            ps.ps_f12_mul_sparse(ptr(wa), ptr(w0), ptr(w2), ptr(w3), ptr(out))
            got = PR.gt_from_words(out)
            assert got == call12(ps.ps_f12_mul, a, dense) == PR.f12_mul(a, dense)


def test_cyclotomic_squaring_and_exponentiation_by_x(ps):
    easy_exp = (P**6 - 1) * (P**2 + 1)
    for a in operands(10, n=3)[3:]:
        m = call12(ps.ps_final_exp_easy, a)
        assert m == PR.f12_pow(a, easy_exp)
        assert call12(ps.ps_f12_cyclotomic_sqr, m) == call12(ps.ps_f12_sqr, m) == PR.f12_mul(m, m)
        assert call12(ps.ps_f12_exp_abs_x, m) == PR.f12_pow(m, PR.X_ABS)
    assert call12(ps.ps_f12_cyclotomic_sqr, PR.F12_ONE) == PR.F12_ONE
    assert call12(ps.ps_final_exp_easy, PR.F12_ZERO) == PR.F12_ZERO      # no division: zero stays zero


def test_final_exponentiation_is_the_integer_power_with_the_stated_c(ps):
    c = ps.ps_final_exp_c()
    assert c == 3 and R % c != 0
    for a in operands(11, n=2)[3:]:
        assert call12(ps.ps_final_exp, a) == PR.f12_pow(a, PR.final_exponent(c))
    w = PC.gt_words(PR.F12_ONE)
    assert ps.ps_f12_is_one(ptr(w)) == 1
    w[70] = 1
    assert ps.ps_f12_is_one(ptr(w)) == 0


# ---- Miller loop steps against the reference line through the same points ----
def affine_of(T):
    """Jacobian (X, Y, Z) over F_p^2 -> affine twist point"""
    zi = PR.f2_inv(T[2])
    zi2 = PR.f2_mul(zi, zi)
    return (PR.f2_mul(T[0], zi2), PR.f2_mul(T[1], PR.f2_mul(zi2, zi)))


def check_line(line, ref_line, yp):
    """the library's line is the reference's times w^3 and a non-zero factor s of F_p^2: s is read off the w^3 coefficient
    (s yp), and then the whole of F_p^12 must agree"""
    l0, l2, l3 = line
    s = PR.f2_scale(l3, pow(yp, -1, P))
    assert s != (0, 0)
    w3s = [(0, 0)] * 3 + [s] + [(0, 0)] * 2
    assert PR.f12_mul(ref_line, w3s) == [l0, (0, 0), l2, l3, (0, 0), (0, 0)]


def step(ps, name, T, p, q=None):
    t = np.concatenate([PC.f2_words(c) for c in T])
    line = np.zeros(36, np.uint64)
    pw = PC.g1_words(p)
    if q is None:
        getattr(ps, name)(ptr(t), ptr(pw), ptr(line))
    else:
        qw = PC.g2_words(q)
        getattr(ps, name)(ptr(t), ptr(qw), ptr(pw), ptr(line))
    return [PC.f2_from_words(t[12 * i:12 * i + 12]) for i in range(3)], [PC.f2_from_words(line[12 * i:12 * i + 12]) for i in range(3)]


def test_doubling_and_addition_steps(ps):
    p, q = PC.g1_mul(0x1234567), PC.g2_mul(0x7654321)
    T = [q[0], q[1], (1, 0)]
    for _ in range(3):   # from Z = 1 and then from the Z the steps leave behind
        before = affine_of(T)
        want, slope = PR.twist_double(before)
        T, line = step(ps, "ps_miller_double", T, p)
        assert affine_of(T) == want
        check_line(line, PR._line(before, slope, p), p[1])
        before = affine_of(T)
        want, slope = PR.twist_add(before, q)
        T, line = step(ps, "ps_miller_add", T, p, q)
        assert affine_of(T) == want
        check_line(line, PR._line(before, slope, p), p[1])
    # the addition step with T = Q (no chord): straight-line arithmetic returns, whatever it returns
    step(ps, "ps_miller_add", [q[0], q[1], (1, 0)], p, q)


def test_one_whole_pairing(ps):
    c = ps.ps_final_exp_c()
    a, b = 0xabcdef0123456789, R - 5
    p, q = PC.g1_mul(a), PC.g2_mul(b)
    out = np.zeros(72, np.uint64)
    pw, qw = PC.g1_words(p), PC.g2_words(q)
    ps.ps_pairing(ptr(pw), ptr(qw), ptr(out))
    got = PR.gt_from_words(out)
    assert got == PR.pairing(p, q, c)                       # the reference's own Miller loop and integer power
    assert got == PR.gt_power(c, a * b)                     # and bilinearity from e(G1, G2)
    ps.ps_miller_loop(ptr(pw), ptr(qw), ptr(out))
    assert PR.f12_pow(PR.gt_from_words(out), PR.final_exponent(c)) == got


def test_point_status(ps):
    g1, g2 = PC.g1_mul(77), PC.g2_mul(78)
    for torsion in (0, 1):
        assert ps.ps_point_status_g1(ptr(PC.g1_words(g1)), torsion) == 0
        assert ps.ps_point_status_g2(ptr(PC.g2_words(g2)), torsion) == 0
        assert ps.ps_point_status_g1(ptr(PC.g1_words((P, g1[1]))), torsion) == 1
        assert ps.ps_point_status_g1(ptr(PC.g1_words((g1[0], 2**384 - 1))), torsion) == 1
        assert ps.ps_point_status_g2(ptr(PC.g2_words(((g2[0][0], P), g2[1]))), torsion) == 1
        assert ps.ps_point_status_g1(ptr(PC.g1_words((g1[0], (g1[1] + 1) % P))), torsion) == 2
        assert ps.ps_point_status_g2(ptr(PC.g2_words((g2[0], (g2[1][0], (g2[1][1] + 1) % P)))), torsion) == 2
        assert ps.ps_point_status_g1(ptr(PC.g1_words(None)), torsion) == 2        # all-zero coordinates are not on the curve
        assert ps.ps_point_status_g2(ptr(PC.g2_words(None)), torsion) == 2
    o1, o2 = PC.g1_outside_torsion(), PC.g2_outside_torsion()
    assert ps.ps_point_status_g1(ptr(PC.g1_words(o1)), 1) == 3 and ps.ps_point_status_g1(ptr(PC.g1_words(o1)), 0) == 0
    assert ps.ps_point_status_g2(ptr(PC.g2_words(o2)), 1) == 3 and ps.ps_point_status_g2(ptr(PC.g2_words(o2)), 0) == 0
    assert ps.ps_point_status_g1(ptr(PC.g1_words(PC.g1_mul(R - 1))), 1) == 0
