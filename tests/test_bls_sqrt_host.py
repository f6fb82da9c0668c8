"""The square roots, the "larger root" predicates and the element decoder of city-rollup_amd/csrc/bls_sqrt.h on the CPU
(tests/sqrtsim: the __host__ __device__ code the unpack kernels run, built for the host) against Python integers. The
formulas here are written independently: Euler's criterion for "has a root", squaring for "is a root", integer comparison
for "larger". No GPU."""
import ctypes

import numpy as np
import pytest

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def ss():
    import simlibs
    return ctypes.CDLL(simlibs.build("sqrtsim"))


def words(*vals):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for v in vals for i in range(6)], dtype=np.uint64)


def value(w):
    return sum(int(x) << (64 * i) for i, x in enumerate(w))


def is_residue(a):
    return a == 0 or pow(a, (P - 1) // 2, P) == 1


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_is_square(a):
    """a^((p^2 - 1) / 2) = norm(a)^((p - 1) / 2): a square of F_p^2 exactly where its norm is a residue of F_p"""
    return is_residue((a[0] * a[0] + a[1] * a[1]) % P)


def rand_fp(rng):
    return int.from_bytes(rng.bytes(64), "little") % P


def fp_sqrt(ss, a):
    out = np.full(6, 7, np.uint64)
    ok = ss.ss_fp_sqrt(words(a).ctypes.data_as(u64p), out.ctypes.data_as(u64p))
    if not ok:
        assert (out == 7).all()
        return None
    return value(out)


def fp2_sqrt(ss, a):
    out = np.full(12, 7, np.uint64)
    ok = ss.ss_fp2_sqrt(words(*a).ctypes.data_as(u64p), out.ctypes.data_as(u64p))
    if not ok:
        assert (out == 7).all()
        return None
    return value(out[:6]), value(out[6:])


def fp_inputs():
    rng = np.random.default_rng(11)
    squares = [pow(rand_fp(rng), 2, P) for _ in range(32)]
    non = []
    while len(non) < 32:
        a = rand_fp(rng)
        if not is_residue(a):
            non.append(a)
    return [0, 1, P - 1] + squares + non


def test_the_exponentiation_and_the_halving(ss):
    rng = np.random.default_rng(3)
    for a in [0, 1, 2, P - 1, P - 2] + [rand_fp(rng) for _ in range(8)]:
        out = np.zeros(6, np.uint64)
        ss.ss_fp_pow_p34(words(a).ctypes.data_as(u64p), out.ctypes.data_as(u64p))
        assert value(out) == pow(a, (P - 3) // 4, P), hex(a)
        ss.ss_fp_half(words(a).ctypes.data_as(u64p), out.ctypes.data_as(u64p))
        assert value(out) * 2 % P == a and value(out) < P, hex(a)


def test_fp_sqrt_exists_exactly_for_residues_and_squares_back(ss):
    assert not is_residue(P - 1)                      # p = 3 mod 4
    n_roots = 0
    for a in fp_inputs():
        r = fp_sqrt(ss, a)
        assert (r is not None) == is_residue(a), hex(a)
        if r is not None:
            assert r < P and r * r % P == a, hex(a)
            n_roots += 1
    assert n_roots == 2 + 32


def test_fp_sign_follows_the_flag_through_the_decoder(ss):
    """x -> (x, y) with y the larger root exactly where 0x80 is set: on the first 24 abscissae of curve points from 1 up"""
    x, found = 0, 0
    while found < 24:
        x += 1
        rhs = (x**3 + 4) % P
        for flag in (0, 0x80):
            raw = bytearray(x.to_bytes(48, "little"))
            raw[47] |= flag
            src = np.frombuffer(bytes(raw), np.uint8).copy()
            xy = np.full(12, 7, np.uint64)
            st = ss.ss_g1_decompress(src.ctypes.data_as(u8p), xy.ctypes.data_as(u64p))
            if not is_residue(rhs):
                assert st == 3 and (xy == 7).all(), x
                continue
            y = value(xy[6:])
            assert st == 0 and value(xy[:6]) == x and y * y % P == rhs, x
            assert (y > (P - y) % P) == bool(flag), x
        found += is_residue(rhs)


def test_fp2_sqrt_exists_exactly_for_squares_and_squares_back(ss):
    rng = np.random.default_rng(12)
    res = pow(rand_fp(rng), 2, P)
    non = P - res                                     # -1 is a non-residue: so is -res
    assert is_residue(res) and not is_residue(non)
    squares = [f2_mul(a, a) for a in [(rand_fp(rng), rand_fp(rng)) for _ in range(32)]]
    non_squares = []
    while len(non_squares) < 16:
        a = (rand_fp(rng), rand_fp(rng))
        if not f2_is_square(a):
            non_squares.append(a)
    inputs = [(0, 0), (1, 0), (res, 0), (non, 0), (0, res), (0, non), (0, 1), (P - 1, 0)] + squares + non_squares
    n_roots = 0
    for a in inputs:
        r = fp2_sqrt(ss, a)
        assert (r is not None) == f2_is_square(a), a
        if r is not None:
            assert r[0] < P and r[1] < P and f2_mul(r, r) == a, a
            n_roots += 1
    assert n_roots == len(inputs) - 16                # every (c, 0) and (0, c) is a square of F_p^2
    r = fp2_sqrt(ss, (non, 0))
    assert r[0] == 0 and r[1] != 0                    # a non-residue of F_p: the root is purely imaginary
    r = fp2_sqrt(ss, (res, 0))
    assert r[1] == 0 and r[0] != 0


def larger1(ss, y):
    return ss.ss_fp_is_larger(words(y).ctypes.data_as(u64p))


def larger2(ss, y):
    return ss.ss_fp2_is_larger(words(*y).ctypes.data_as(u64p))


def test_larger_predicates(ss):
    assert larger1(ss, 0) == 0 and larger2(ss, (0, 0)) == 0
    rng = np.random.default_rng(13)
    for y in [1, (P - 1) // 2, (P + 1) // 2, 2, P - 2] + [rand_fp(rng) for _ in range(8)]:
        got = (larger1(ss, y), larger1(ss, P - y))
        assert got == ((1, 0) if y > P - y else (0, 1)), hex(y)
    assert (larger1(ss, (P - 1) // 2), larger1(ss, (P + 1) // 2)) == (0, 1)
    cases = [(0, 1), (1, 0), (P - 1, 0), ((P - 1) // 2, 0), (5, (P - 1) // 2), (P - 5, (P - 1) // 2)]
    cases += [(rand_fp(rng), rand_fp(rng)) for _ in range(8)]
    for y in cases:
        neg = ((P - y[0]) % P, (P - y[1]) % P)
        want = y[1] > neg[1] if y[1] != neg[1] else y[0] > neg[0]
        assert (larger2(ss, y), larger2(ss, neg)) == ((1, 0) if want else (0, 1)), y
    # c1 = 0: the decision falls to c0
    assert (larger2(ss, (1, 0)), larger2(ss, (P - 1, 0))) == (0, 1)


def test_g2_decoder_classes_and_sign(ss):
    """the element decoder on F_p^2: flags, range, no-point, and both signs on the first abscissae (k, 1) of twist points"""
    def run(x0, x1, flag0=0, flag1=0):
        raw = bytearray(x0.to_bytes(48, "little") + x1.to_bytes(48, "little"))
        raw[47] |= flag0
        raw[95] |= flag1
        src = np.frombuffer(bytes(raw), np.uint8).copy()
        xy = np.full(24, 7, np.uint64)
        st = ss.ss_g2_decompress(src.ctypes.data_as(u8p), xy.ctypes.data_as(u64p))
        if st:
            assert (xy == 7).all()
            return st, None
        return 0, ((value(xy[:6]), value(xy[6:12])), (value(xy[12:18]), value(xy[18:])))

    seen = {0: 0, 3: 0}
    for k in range(1, 17):
        x = (k, 1)
        rhs = f2_mul(f2_mul(x, x), x)
        rhs = ((rhs[0] + 4) % P, (rhs[1] + 4) % P)
        for flag in (0, 0x80):
            st, pt = run(k, 1, flag1=flag)
            assert st == (0 if f2_is_square(rhs) else 3), k
            seen[st] += 1
            if st == 0:
                y = pt[1]
                neg = ((P - y[0]) % P, (P - y[1]) % P)
                assert pt[0] == x and f2_mul(y, y) == rhs
                assert (y[1] > neg[1] if y[1] != neg[1] else y[0] > neg[0]) == bool(flag), k
    assert seen[0] and seen[3]
    assert run(1, 1, flag1=0x40)[0] == 1 and run(1, 1, flag0=0x40)[0] == 1 and run(1, 1, flag0=0x80)[0] == 1
    assert run(P, 1)[0] == 2 and run(1, P)[0] == 2
    assert run(P, 1, flag1=0x40)[0] == 1              # the smallest class that applies
