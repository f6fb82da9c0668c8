"""The arithmetic primitives of city-rollup_amd/csrc (gl.h, poseidon.h, ntt16.h, ext3.h, bls12_381.h, bls12_381_fr.h, the one-limb
product of r1cs.h) executed ON THE DEVICE one by one, at the operand tables of the CPU unit tests (tests/arith_cases.py,
tests/product_chain.py, tests/rare_paths.py, tests/bls_rare_paths.py), under every lane pattern of rare_paths.patterns. tests/devsim
holds the device twin (`ds_*`) of every hostsim wrapper (`hs_*`), compiled with the product's flags. Two exact comparisons each:
against Python integers / Fractions, and bit for bit against the host instantiation of the same lines."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import arith_cases as AC
import bls_rare_paths as B
import oracle_lib as O
import product_chain as C
import rare_paths as R

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
P, M64, EPS = AC.P, AC.M64, AC.EPS
CHUNK = 2048
U64, U32, F64, I32 = np.uint64, np.uint32, np.float64, np.int32
TWO = ("every_lane", "alternate")


class Libs:
    pass


@pytest.fixture(scope="module")
def L():
    import simlibs
    so = simlibs.build_all(["devsim_gl", "devsim_bls"])
    lib = Libs()
    lib.gl, lib.bls = ctypes.CDLL(so["devsim_gl"]), ctypes.CDLL(so["devsim_bls"])
    lib.hs, lib.rn = ctypes.CDLL(simlibs.build("hostsim")), ctypes.CDLL(simlibs.build("renorm_hostsim"))
    u64, u32, dbl = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double
    for name, args in (("hs_mul", [u64] * 2), ("hs_mul_lazy", [u64] * 2), ("hs_add", [u64] * 2), ("hs_sub", [u64] * 2), ("hs_gl_op1", [ctypes.c_int, u64]),
                       ("hs_gl_op2", [ctypes.c_int, u64, u64]), ("hs_mul_add_lazy", [u64] * 3), ("hs_fold_top", [u64, u32]),
                       ("hs_reduce128_lazy", [ctypes.c_int, u64, u64, u32]), ("hs_mul_pow2", [u64, ctypes.c_int]), ("hs_recombine_d", [dbl, dbl, u64])):
        getattr(lib.hs, name).restype = u64
        getattr(lib.hs, name).argtypes = args
    lib.hs.hs_gl_chain.argtypes = [ctypes.c_int, u64, u64, u64, ctypes.c_void_p]
    lib.hs.hs_mul_paths.argtypes = [u64, u64]
    lib.rn.hs_rn_recombine.restype = u64
    lib.rn.hs_rn_recombine.argtypes = [dbl, dbl, ctypes.c_int, ctypes.c_int]
    return lib


class N(int):
    """an element count (size_t in the ABI)"""


def ptr(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.c_void_p)


def call(fn, *args):
    """a ds_* entry (returns the hipError_t) or an hs_* entry that works on arrays"""
    conv = [ptr(a) if isinstance(a, np.ndarray) else ctypes.c_size_t(a) if isinstance(a, N) else ctypes.c_uint32(a) if a > 0x7FFFFFFF else ctypes.c_int(a)
            for a in args]
    fn.restype = ctypes.c_int
    return fn(*conv)


def dev(fn, *args):
    rc = call(fn, *args)
    assert rc == 0, "%s: hipError_t %d" % (fn.__name__, rc)


def u64(vals):
    return np.array([int(v) for v in vals], dtype=U64)


def first_bad(ok, idx):
    bad = np.nonzero(~ok.reshape(ok.shape[0], -1).all(axis=1))[0]
    return "element %d = case %d" % (bad[0], idx[bad[0]]) if bad.size else ""


def run_table(launch, inputs, expect, out_shape=(), out_dtype=U64, patterns=R.PATTERNS, inplace=False):
    """The cases (first axis of every array of `inputs`) laid out over launches of a few thousand elements: under each lane pattern
    the active lanes walk through the cases, the others hold other cases and must keep the sentinel (in place: their input).
    launch(tiled inputs, out, mask, n). expect: [("eq", array)] the output exactly (words bit for bit, doubles by value:
    a zero has no sign to get wrong), [("mod", array)] modulo p."""
    ncases = inputs[0].shape[0]
    for start in range(0, ncases, CHUNK):
        m = min(CHUNK, ncases - start)
        n = max(1024, 2 * m) + 37
        for pi, name in enumerate(patterns):
            mask = R.patterns(n)[name]
            act = np.nonzero(mask)[0]
            idx = start + (np.arange(n) * 7 + 3) % m
            idx[act] = start + (np.arange(act.size) + 17 * pi) % m
            tiled = [np.ascontiguousarray(x[idx]) for x in inputs]
            if inplace:
                out = tiled[0]
                before = out.copy()
            else:
                out = np.empty((n,) + tuple(out_shape), out_dtype)
                out.view(np.uint8)[...] = 0xA5
            launch(tiled, out, mask.astype(np.uint8), N(n))
            for kind, want in expect:
                w = want[idx[mask]]
                ok = (out[mask] == w) if kind == "eq" else (out[mask] % U64(P) == w)
                assert ok.all(), (name, kind, first_bad(ok, idx[mask]))
            if inplace:
                assert (out[~mask] == before[~mask]).all(), (name, "a lane the mask switches off wrote")
            else:
                assert (out[~mask].view(np.uint8) == 0xA5).all(), (name, "a lane the mask switches off wrote")


def host_each(fn, *cols):
    """the scalar hs_* entry over the cases"""
    return u64([fn(*[int(v) for v in row]) for row in zip(*cols)])


# ---- gl.h: the product chain ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def witness():
    """every class and corner of product_chain under every lane pattern, the addends of mul_add_lazy, and the exact lazy results"""
    a, b, masks = C.witness_array(n=512)
    rng = np.random.default_rng(77)
    c = rng.integers(0, 1 << 64, a.size, dtype=U64)
    for i in range(0, a.size, 2):             # every second element: an addend at a bound, or around the wrap of lo + c
        lo = (int(a[i]) * int(b[i])) & M64
        c[i] = (AC.MUL_ADD_C + [(-lo) & M64, (-lo - 1) & M64, M64 - lo])[(i // 2) % 8]
    lazy = u64([C.chain(x, y).lazy for x, y in zip(a, b)])
    lazy_add = u64([C.chain(x, y, z).lazy for x, y, z in zip(a, b, c)])
    planted = np.zeros(a.size, bool)
    for key, name, off, mask in masks:
        planted[off:off + mask.size] = mask
        for i in np.nonzero(mask)[0][:4]:
            ch = C.chain(a[off + i], b[off + i])
            assert key in (ch[:4], ch.corner)
    return a, b, c, lazy, lazy_add, planted


@pytest.mark.parametrize("op", ["mul_lazy", "mul_add_lazy", "mul"])
def test_product_classes(L, witness, op):
    a, b, c, lazy, lazy_add, planted = witness
    n = N(a.size)
    if op == "mul_lazy":
        want, host = lazy, host_each(L.hs.hs_mul_lazy, a, b)
    elif op == "mul_add_lazy":
        want, host = lazy_add, host_each(L.hs.hs_mul_add_lazy, a, b, c)
    else:
        want, host = lazy % U64(P), host_each(L.hs.hs_mul, a, b)
    assert (host == want).all()
    assert (want % U64(P) == u64([(int(x) * int(y) + (int(z) if op == "mul_add_lazy" else 0)) % P for x, y, z in zip(a, b, c)])).all()
    for mask in (planted, np.ones(a.size, bool), ~planted):
        out = np.full(a.size, 0xA5A5A5A5A5A5A5A5, U64)
        m8 = mask.astype(np.uint8)
        if op == "mul_add_lazy":
            dev(L.gl.ds_mul_add_lazy, a, b, c, out, m8, n)
        else:
            dev(getattr(L.gl, "ds_" + op), a, b, out, m8, n)
        ok = out[mask] == want[mask]
        assert ok.all(), first_bad(ok, np.nonzero(mask)[0])
        assert (out[~mask] == U64(0xA5A5A5A5A5A5A5A5)).all()


def test_mul_add_lazy_addends_and_lazy_operands(L):
    la, lb = AC.lazy_operands(64, 3)
    pairs = [(x, y) for x in C.EDGE for y in C.EDGE] + list(zip(la, lb))
    cases = AC.mul_add_cases(pairs)
    a, b, c = (u64(col) for col in zip(*cases))
    want = u64([C.chain(x, y, z).lazy for x, y, z in cases])
    assert (want % U64(P) == u64([(x * y + z) % P for x, y, z in cases])).all()
    assert (host_each(L.hs.hs_mul_add_lazy, a, b, c) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_mul_add_lazy, t[0], t[1], t[2], o, m, n), [a, b, c], [("eq", want)])
    # the plain products with both operands lazy, in [p, 2^64)
    la, lb = AC.lazy_operands(600, 4)
    lazy = u64([C.chain(x, y).lazy for x, y in zip(la, lb)])
    assert (host_each(L.hs.hs_mul_lazy, la, lb) == lazy).all() and (host_each(L.hs.hs_mul, la, lb) == lazy % U64(P)).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_mul_lazy, t[0], t[1], o, m, n), [la, lb], [("eq", lazy)])
    run_table(lambda t, o, m, n: dev(L.gl.ds_mul, t[0], t[1], o, m, n), [la, lb], [("eq", lazy % U64(P)), ("eq", u64([int(x) * int(y) % P for x, y in zip(la, lb)]))])


@pytest.mark.parametrize("form", [0, 1])
def test_reduce128_lazy_tables(L, form):
    cases = [r for r in AC.reduce128_cases() if form or not r[2]]
    lo, hi = u64([r[0] for r in cases]), u64([r[1] for r in cases])
    cy = np.array([r[2] for r in cases], U32)
    paths = [R.reduce_paths(r[0], r[1]) for r in cases]
    want = u64([p.lazy for p in paths])
    assert sum(p.borrow for p in paths) > 50 and sum(p.fold_wrap for p in paths) > 50 and sum(p.borrow and p.fold_wrap for p in paths) > 5
    assert (want % U64(P) == u64([(r[0] + (r[1] << 64)) % P for r in cases])).all()
    assert (u64([L.hs.hs_reduce128_lazy(form, r[0], r[1], r[2]) for r in cases]) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_reduce128_lazy, form, t[0], t[1], t[2], o, m, n), [lo, hi, cy], [("eq", want)])


def test_fold_top_around_the_wrap(L):
    cases = AC.fold_top_cases()
    lo, top = u64([r[0] for r in cases]), np.array([r[1] for r in cases], U32)
    want = u64([AC.fold_top_py(*r) for r in cases])
    assert (want % U64(P) == u64([(l + (t << 64)) % P for l, t in cases])).all()
    assert any(l + t * EPS >> 64 for l, t in cases) and any(t and not l + t * EPS >> 64 for l, t in cases)
    assert (u64([L.hs.hs_fold_top(*r) for r in cases]) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_fold_top, t[0], t[1], o, m, n), [lo, top], [("eq", want)])


def add_lazy_py(a, b):
    s = a + b
    if s >> 64:
        s = (s & M64) + EPS
        if s >> 64:
            s = (s & M64) + EPS
    return s


def test_field_ops_at_the_edges(L):
    a, b = (u64(col) for col in zip(*AC.GL_EDGE_PAIRS))
    canonical = (a < U64(P)) & (b < U64(P))
    ints = lambda f: u64([f(int(x), int(y)) for x, y in zip(a, b)])
    for op, name, f in ((2, "ds_add", lambda x, y: (x + y) % P), (3, "ds_sub", lambda x, y: (x - y) % P)):
        host = host_each(L.hs.hs_gl_op2, [op] * a.size, a, b)
        assert (host[canonical] == ints(f)[canonical]).all()
        # canonical pairs against the integers; all pairs (p and 2^64 - 1 are outside the contract) bit for bit against the host
        run_table(lambda t, o, m, n: dev(getattr(L.gl, name), t[0], t[1], o, m, n), [a[canonical], b[canonical]], [("eq", ints(f)[canonical])])
        run_table(lambda t, o, m, n: dev(L.gl.ds_gl_op2, op, t[0], t[1], o, m, n), [a, b], [("eq", host)])
    want = ints(add_lazy_py)
    assert (want % U64(P) == ints(lambda x, y: (x + y) % P)).all() and (host_each(L.hs.hs_gl_op2, [4] * a.size, a, b) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_gl_op2, 4, t[0], t[1], o, m, n), [a, b], [("eq", want)])
    # add_const_lazy: any u64 plus a canonical constant
    la = u64([x for x in AC.LAZY_EXTREMES for _ in range(4)])
    lc = u64([c for _ in AC.LAZY_EXTREMES for c in (0, 1, P - 1, R.RC[5])])
    want = u64([add_lazy_py(int(x), int(c)) for x, c in zip(la, lc)])
    assert (host_each(L.hs.hs_gl_op2, [6] * la.size, la, lc) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_gl_op2, 6, t[0], t[1], o, m, n), [la, lc], [("eq", want)])
    # one operand: canon of any u64, neg / sqr / pow7 / inv of canonical values, sbox_lazy of any u64
    x = u64(AC.GL_EDGE + AC.LAZY_EXTREMES + AC.POW_BASES)
    xc = x[x < U64(P)]

    def sbox(v):
        x2 = C.chain(v, v).lazy
        x4, x3 = C.chain(x2, x2).lazy, C.chain(v, x2).lazy
        return C.chain(x3, x4).lazy
    for op, arg, f in ((0, x, lambda v: v % P), (1, xc, lambda v: -v % P), (2, xc, lambda v: pow(v, P - 2, P)), (3, xc, lambda v: v * v % P),
                       (5, xc, lambda v: pow(v, 7, P)), (4, x, sbox)):
        want = u64([f(int(v)) for v in arg])
        if op == 4:
            assert (want % U64(P) == u64([pow(int(v), 7, P) for v in arg])).all()
        assert (host_each(L.hs.hs_gl_op1, [op] * arg.size, arg) == want).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_gl_op1, op, t[0], o, m, n), [arg], [("eq", want)])
    pb, pe = (u64(col) for col in zip(*[(v, e) for v in AC.POW_BASES for e in AC.POW_EXPONENTS]))
    want = u64([pow(int(v), int(e), P) for v, e in zip(pb, pe)])
    assert (host_each(L.hs.hs_gl_op2, [5] * pb.size, pb, pe) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_gl_op2, 5, t[0], t[1], o, m, n), [pb, pe], [("eq", want)])


def test_ext_mul_and_mul_paths(L):
    rng = np.random.default_rng(5)
    x = rng.integers(0, P, (300, 2), dtype=U64)
    y = rng.integers(0, P, (300, 2), dtype=U64)
    edge = [0, 1, P - 1, 7, EPS, 1 << 63]
    for i, (p, q) in enumerate((p, q) for p in edge for q in edge):
        x[i], y[i] = (p, q), (q, P - 1 - p if p else 0)
    want = np.array([R.ext_mul_py((int(a[0]), int(a[1])), (int(b[0]), int(b[1]))) for a, b in zip(x, y)], dtype=U64)
    host = np.zeros_like(want)
    for i in range(len(x)):
        L.hs.hs_ext_mul(ptr(x[i].copy()), ptr(y[i].copy()), ctypes.c_void_p(host[i].ctypes.data))
    assert (host == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_ext_mul, t[0], t[1], o, m, n), [x, y], [("eq", want)], out_shape=(2,))
    # which paths a product takes, from the 128-bit restatement compiled for the device (reduce128_lazy(lo, hi) against its pieces)
    w, _ = C.witnesses()
    pairs = [pq for key in C.CLASSES + C.CORNERS for pq in w[key]] + [(a, b) for a in C.EDGE for b in C.EDGE]
    a, b = (u64(col) for col in zip(*pairs))
    pp = [R.mul_paths(p, q) for p, q in pairs]
    want = np.array([p.borrow | p.fold_wrap << 1 | p.lazy_ge_p << 2 for p in pp], I32)
    assert (np.array([L.hs.hs_mul_paths(int(p), int(q)) for p, q in pairs], I32) == want).all() and set(want) >= {0, 1, 2, 3, 4}
    run_table(lambda t, o, m, n: dev(L.gl.ds_mul_paths, t[0], t[1], o, m, n), [a, b], [("eq", want)], out_dtype=I32)


@pytest.mark.parametrize("which", [0, 1])
def test_product_chains_on_one_thread(L, witness, which):
    """three products per thread with all results kept: the carries and borrow masks of several products live at once. Each slot
    sees every class: the witness pairs go to (a, b), then (b, c), then (c, a)."""
    wa, wb, wc, _, _, planted = witness
    sel = np.nonzero(planted)[0][::3][:4000]           # the planted pairs, every class and corner
    wa, wb, wc = wa[sel], wb[sel], wc[sel]
    for rot in range(3):
        a, b, c = ((wa, wb, wc), (wc, wa, wb), (wb, wc, wa))[rot]
        if which == 0:
            want = np.stack([u64([C.chain(x, y).lazy for x, y in zip(a, b)]), u64([C.chain(y, z, x).lazy for x, y, z in zip(a, b, c)]),
                             u64([int(z) * int(x) % P for x, z in zip(a, c)])], axis=1)
        else:
            r0, r1 = [C.chain(x, y).lazy for x, y in zip(a, b)], [C.chain(z, x).lazy for x, z in zip(a, c)]
            want = np.stack([u64(r0), u64(r1), u64([p * q % P for p, q in zip(r0, r1)])], axis=1)
        host = np.zeros_like(want)
        for i in range(len(a)):
            L.hs.hs_gl_chain(which, int(a[i]), int(b[i]), int(c[i]), ctypes.c_void_p(host[i].ctypes.data))
        assert (host == want).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_gl_chain, which, t[0], t[1], t[2], o, m, n), [a, b, c], [("eq", want)], out_shape=(3,),
                  patterns=R.PATTERNS if rot == 0 else TWO)


# ---- ntt16.h ---------------------------------------------------------------------------------------------------------------------
def test_mul_pow2_all_192_shifts(L):
    vals = AC.mul_pow2_operands()
    x = u64([v for k in range(192) for v in vals])
    k = np.array([k for k in range(192) for _ in vals], I32)
    want = u64([(int(v) << int(s)) % P for v, s in zip(x, k)])
    assert (u64([L.hs.hs_mul_pow2(int(v), int(s)) for v, s in zip(x, k)]) == want).all()
    run_table(lambda t, o, m, n: dev(L.gl.ds_mul_pow2, t[0], t[1], o, m, n), [x, k], [("eq", want)], patterns=("every_lane", "alternate", "lane63"))


def test_radix16_register_butterfly(L):
    rng = np.random.default_rng(6)
    x = rng.integers(0, P, (40, 16), dtype=U64)
    x[0] = AC.round16_inputs()
    x[1] = P - 1
    x[2] = 0
    x[3] = [P - 1, 0] * 8
    inv16 = pow(16, P - 2, P)
    for inverse in (0, 1):
        if inverse:          # the same network with omega^-1, no 1/n scaling
            want = np.array([[int(v) * 16 % P for v in O.bit_reverse(O.intt(row))] for row in x], dtype=U64)
            assert all(int(v) * inv16 % P == int(w) for v, w in zip(want[0], O.bit_reverse(O.intt(x[0]))))
        else:
            want = np.array([O.bit_reverse(O.ntt(row)) for row in x], dtype=U64)
        host = x.copy()
        for row in host:
            L.hs.hs_round16(ctypes.c_void_p(row.ctypes.data), inverse)
        assert (host == want).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_round16, o, inverse, m, n), [x], [("eq", want)], inplace=True)


# ---- poseidon.h: the double-precision planes ---------------------------------------------------------------------------------------
def test_renorm_against_exact_rationals(L):
    cases = AC.renorm_cases()
    U, LIM = AC.U, AC.LIM
    scaled = np.array([[float(l * U), float(h * U)] for l, h in cases])
    plain = np.array([[float(l), float(h)] for l, h in cases])
    want32, ties = [], 0
    for l, h in cases:
        Ls, Hs = l * U, h * U
        assert AC.representable(Ls) and AC.representable(Hs)
        wl, wh, c, t = AC.exact_renorm32(Ls, Hs)
        assert abs(wl) <= LIM * U and abs(wh) <= LIM * U
        d = ((wl + (1 << 32) * wh) - (Ls + (1 << 32) * Hs)) / U
        assert d.denominator == 1 and d.numerator == -t * P
        ties += (Ls - Ls.numerator // Ls.denominator == Fraction(1, 2)) + ((Hs + c * U) - (Hs + c * U).numerator // (Hs + c * U).denominator == Fraction(1, 2))
        want32.append([float(wl), float(wh)])
        assert Fraction(want32[-1][0]) == wl and Fraction(want32[-1][1]) == wh
    assert ties >= 40
    want32 = np.array(want32)
    want1 = want32 * 2.0 ** 32                   # the same limbs in units of 1 (exact: only the exponents change)
    for which, arr, want in ((0, scaled, want32), (1, plain, want1)):
        host = np.zeros_like(arr)
        for i in range(len(arr)):
            L.rn.hs_rn_renorm(which, ctypes.c_void_p(arr[i].ctypes.data), ctypes.c_void_p(host[i].ctypes.data))
        assert (host.view(U64) == want.view(U64)).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_rn_renorm, which, t[0], o, m, n), [arr], [("eq", want)], out_shape=(2,), out_dtype=F64)
    run_table(lambda t, o, m, n: dev(L.gl.ds_renorm_d, t[0], o, m, n), [plain], [("eq", want1)], out_shape=(2,), out_dtype=F64, patterns=TWO)


def test_recombine_all_four_constant_tables(L):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "city-rollup_amd", "csrc"))
    import gen_tables
    dk, dlast = gen_tables.plane_constants(gen_tables.round_constants(), first_too=True)
    limbs = AC.recombine_limbs()
    rows = [(t, i, l, h, c) for t, consts in ((0, dk), (1, dlast)) for i, c in enumerate(consts) for l, h in limbs]
    for scale in (0, 2):        # tables 0 / 1: limbs in units of 1; tables 2 / 3: the same limbs in units of 2^32
        f = Fraction(1) if scale == 0 else AC.U
        lf = np.array([float(Fraction(r[2]) * f) for r in rows])
        hf = np.array([float(Fraction(r[3]) * f) for r in rows])
        table = np.array([r[0] + scale for r in rows], I32)
        idx = np.array([r[1] for r in rows], I32)
        host = u64([L.rn.hs_rn_recombine(float(a), float(b), int(t), int(i)) for a, b, t, i in zip(lf, hf, table, idx)])
        if scale == 0:
            unscaled = host
        else:
            assert (host == unscaled).all(), "scaled and unscaled constants disagree"
        mod = u64([(l + (h << 32) + c) % P for _, _, l, h, c in rows])
        run_table(lambda t, o, m, n: dev(L.gl.ds_rn_recombine, t[0], t[1], t[2], t[3], o, m, n), [lf, hf, table, idx], [("eq", host), ("mod", mod)])
    ll, hh, cc = (np.array([float(r[k]) for r in AC.RECOMBINE_CONST_CASES]) for k in (0, 1, 2))
    cc = u64([r[2] for r in AC.RECOMBINE_CONST_CASES])
    host = u64([L.hs.hs_recombine_d(float(l), float(h), int(c)) for l, h, c in AC.RECOMBINE_CONST_CASES])
    mod = u64([(l + (h << 32) + c + AC.RECOMBINE_OFFSET) % P for l, h, c in AC.RECOMBINE_CONST_CASES])
    run_table(lambda t, o, m, n: dev(L.gl.ds_recombine_d, t[0], t[1], t[2], o, m, n), [ll, hh, cc], [("eq", host), ("mod", mod)])


def dom_host(L, op, s):
    out = np.zeros((len(s), 12))
    for i in range(len(s)):
        L.hs.hs_dom_d(op, ctypes.c_void_p(s[i].ctypes.data), ctypes.c_void_p(out[i].ctypes.data))
    return out


def pad13(a):
    return np.ascontiguousarray(np.hstack([a, np.zeros((len(a), 1))]))


def test_layer_identities_on_the_device(L):
    """T^-1' . K . T is the MDS without its diagonal, T . T^-1' scales by (4, 4, 2), the scaled products take the state divided by
    (4, 4, 2) (quarter and half integers), and leaving in units of 2^32 only moves the exponents; then one whole layer on lazy
    states, integer planes and double-precision planes."""
    rng, vectors = AC.dom_vectors()
    s = pad13(np.array(vectors, dtype=F64))
    Cm = AC.MDS_C
    stage = {}

    def through(op, inp, want):
        host = dom_host(L, op, inp)
        assert (host.view(U64) == want.view(U64)).all() or (host == want).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_dom_d, op, t[0], o, m, n), [inp], [("eq", host)], out_shape=(12,), out_dtype=F64, patterns=TWO + ("lane63",))
        return host
    u = dom_host(L, 0, s)
    o = dom_host(L, 1, pad13(u))
    y = np.array([[float(sum(Cm[i] * v[(i + r) % 12] for i in range(12))) for r in range(12)] for v in vectors])
    through(0, s, u)
    through(1, pad13(u), o)
    through(3, pad13(o), y)                                              # the circulant, exactly
    scale = np.array([4.0] * 6 + [2.0] * 6)
    through(0, pad13(y), o * scale)
    assert (y[:, 0] == o[:, 0] + o[:, 3] + o[:, 6]).all()
    w = u / scale                                                          # the stored form: quarter / half integers, exact
    through(2, pad13(w), o)
    through(4, pad13(w), o * 2.0 ** -32)
    through(5, pad13(u), o * 2.0 ** -32)
    states = u64([v for st in AC.lazy_states(rng) for v in st]).reshape(-1, 12)
    want = np.array([AC.mds_py([int(v) for v in st]) for st in states], dtype=U64)
    for which in (0, 1):
        host = states.copy()
        for row in host:
            L.hs.hs_mds_layer(ctypes.c_void_p(row.ctypes.data), which)
        assert (host == want).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_mds_layer, o, which, m, n), [states], [("eq", want)], inplace=True)
    # one 22-bit limb plane of the integer form
    rng = np.random.default_rng(1)
    sl = rng.integers(0, 1 << 22, (200, 12), dtype=U32)
    sl[0] = (1 << 22) - 1
    want = np.array([[sum(Cm[i] * int(v[(i + r) % 12]) for i in range(12)) + (8 * int(v[0]) if r == 0 else 0) for r in range(12)] for v in sl], dtype=U32)
    run_table(lambda t, o, m, n: dev(L.gl.ds_mds_limb, t[0], o, m, n), [sl], [("eq", want)], out_shape=(12,), out_dtype=U32, patterns=TWO)


def test_worst_case_vectors_on_the_device(L):
    """every output component of dom_mul_d<true>, dom_mul2_d and dom_next_z at the largest magnitude the stated bounds allow: the
    exact rational result is a double and the device returns it"""
    cases = AC.worst_case_vectors()
    for op in (2, 6, 7):
        rows = [c for c in cases if c[0] == op]
        exact = [AC.dom_exact(op, c[1]) for c in rows]
        assert all(AC.representable(v) for e in exact for v in e) and all(e[c[2]] == c[3] for e, c in zip(exact, rows))
        s = np.array([[float(v) for v in c[1]] for c in rows])
        want = np.array([[float(v) for v in e] for e in exact])
        assert (dom_host(L, op, s) == want).all()
        run_table(lambda t, o, m, n: dev(L.gl.ds_dom_d, op, t[0], o, m, n), [s], [("eq", want)], out_shape=(12,), out_dtype=F64)


# ---- poseidon.h: the permutation forms ---------------------------------------------------------------------------------------------
PERMUTE, ABSORB, SQUEEZE, NODE, TEXTBOOK = range(5)
LIVE = {PERMUTE: (slice(0, 12), True), ABSORB: (slice(8, 12), False), SQUEEZE: (slice(0, 4), True), NODE: (slice(0, 4), True)}


@pytest.fixture(scope="module")
def states():
    st = AC.input_states()
    return st, O.permute_many(st % U64(P)).reshape(-1, 12), O.permute_many(np.hstack([st[:, :8], np.zeros((len(st), 4), U64)]) % U64(P)).reshape(-1, 12)


@pytest.mark.parametrize("form", [PERMUTE, ABSORB, SQUEEZE, NODE], ids=["permute", "permute_absorb", "permute_squeeze", "permute_node"])
def test_permutation_forms_on_the_device(L, states, form):
    st, want_all, want_node = states
    st = st.copy()
    want = want_all
    if form == NODE:                 # a tree node declares its capacity zero: what the words hold is never read
        want = want_node
        st[1::2, 8:] = U64(0xDEADBEEFDEADBEEF)
        st[::2, 8:] = 0
    live, canonical = LIVE[form]
    ref_in = st.copy()
    if form == NODE:
        ref_in[:, 8:] = 0
    rep = np.ascontiguousarray(np.tile(ref_in, (4, 1)))          # 640 states: three workgroups
    text = rep.copy()
    dev(L.gl.ds_permute, text, N(len(text)), TEXTBOOK)
    assert (text == np.tile(want, (4, 1))).all()
    host = st.copy()
    assert call(L.rn.hs_rn_permute, host, N(len(host)), form) == 0
    got = np.ascontiguousarray(np.tile(st, (4, 1)))
    dev(L.gl.ds_permute, got, N(len(got)), form)
    assert (got == np.tile(host, (4, 1))).all(), "host and device differ"
    if canonical:
        assert (got[:, live] == np.tile(want, (4, 1))[:, live]).all()
    else:
        assert ((got[:, live] % U64(P)) == np.tile(want, (4, 1))[:, live]).all()
    expect = [("eq", host)]
    run_table(lambda t, o, m, n: dev(L.gl.ds_rn_permute, o, n, form, m), [st], expect, inplace=True)


def test_other_permutation_entries_and_17_chained_absorbs(L, states):
    st, want_all, _ = states
    for name, how in (("poseidon_permute", "eq"), ("poseidon_permute_textbook", "eq"), ("poseidon_permute_lazy", "mod")):
        host = st.copy()
        getattr(L.hs, "hs_" + name)(ptr(host), ctypes.c_size_t(len(host)))
        run_table(lambda t, o, m, n: dev(getattr(L.gl, "ds_" + name), o, n, m), [st], [("eq", host)], inplace=True, patterns=TWO)
        assert ((host % U64(P)) == want_all).all() if how == "mod" else (host == want_all).all()
    # the middle of a 135-column leaf: 17 capacity-only permutations, the lazy capacity carried from one to the next
    n, rep = 24, 25
    chunks = AC.absorb_chunks(n)
    a = np.zeros((n * rep, 12), U64)
    b = a.copy()
    h = np.zeros((n, 12), U64)
    b2 = np.zeros((n, 12), U64)
    for c in range(17):
        a[:, :8] = np.tile(chunks[c], (rep, 1))
        b[:, :8] = np.tile(chunks[c], (rep, 1))
        h[:, :8] = chunks[c]
        dev(L.gl.ds_permute, a, N(len(a)), ABSORB)
        dev(L.gl.ds_permute, b, N(len(b)), TEXTBOOK)
        assert call(L.rn.hs_rn_permute, h, N(n), ABSORB) == 0
        b2[:, :8] = chunks[c] % U64(P)
        b2 = O.permute_many(b2).reshape(-1, 12)
        assert (a[:, 8:] == np.tile(h, (rep, 1))[:, 8:]).all(), c
        assert ((a[:, 8:] % U64(P)) == b[:, 8:]).all(), c
        assert (b == np.tile(b2, (rep, 1))).all(), c


# ---- ext3.h ----------------------------------------------------------------------------------------------------------------------
def test_cubic_extension(L):
    import air_programs as A
    cases = AC.cubic_cases()
    assert any(m == A.CUBIC_MODULUS for m, _, _ in cases) and any(m == (1, 1) for m, _, _ in cases)
    m, a, b = (np.array([c[k] for c in cases], dtype=U64) for k in range(3))
    X = (0, 1, 0)
    norm = [AC.cubic_norm_py(c[0], c[1]) for c in cases]
    assert all(norm[i] == 0 for i, c in enumerate(cases) if c[0] == AC.REDUCIBLE_MODULUS and c[1] in AC.ZERO_NORM_ELEMENTS)

    def host(op):
        out = np.zeros((len(cases), 4), U64)
        out[:, 3] = U64(0xA5A5A5A5A5A5A5A5)
        for i in range(len(cases)):
            L.hs.hs_cubic(op, ctypes.c_void_p(m[i].ctypes.data), ctypes.c_void_p(a[i].ctypes.data), ctypes.c_void_p(b[i].ctypes.data), ctypes.c_void_p(out[i].ctypes.data))
        return out
    outs = {}
    for op in (0, 1, 2, 3):
        h = host(op)
        run_table(lambda t, o, mk, n: dev(L.gl.ds_cubic, op, t[0], t[1], t[2], o, mk, n), [m, a, b], [("eq", h)], out_shape=(4,))
        outs[op] = [[int(v) for v in row] for row in h]
    for i, (mm, aa, bb) in enumerate(cases):
        assert tuple(outs[0][i][:3]) == AC.cubic_mul_py(mm, aa, bb)
        assert tuple(outs[2][i][:3]) == AC.cubic_mul_py(mm, aa, X)
        adj = tuple(outs[3][i][:3])
        assert outs[3][i][3] == norm[i] and AC.cubic_mul_py(mm, aa, adj) == (norm[i], 0, 0)
        inv = tuple(outs[1][i][:3])
        assert inv == (0, 0, 0) if norm[i] == 0 else AC.cubic_mul_py(mm, aa, inv) == (1, 0, 0)


def test_batch_inverse_of_a_zero_norm_element():
    """a reducible modulus: a non-zero element of norm 0 has no inverse and maps to zero (ext3.h), in the kernel as in the oracle"""
    import cityprover
    rng = np.random.default_rng(9)
    prover = cityprover.Prover(0)
    try:
        for count, n in ((3, 300), (9, 70)):
            cols = rng.integers(0, P, (3 * count, n), dtype=U64)
            for k, e in enumerate(AC.ZERO_NORM_ELEMENTS):
                cols[3 * (k % count):3 * (k % count) + 3, (7 * k + 1) % n] = e
            want = O.cubic_batch_inverse(AC.REDUCIBLE_MODULUS, cols)
            for k, e in enumerate(AC.ZERO_NORM_ELEMENTS):
                assert (want[3 * (k % count):3 * (k % count) + 3, (7 * k + 1) % n] == 0).all()
            assert (cityprover.cubic_batch_inverse(prover, AC.REDUCIBLE_MODULUS, cols) == want).all()
    finally:
        prover.close()


# ---- BLS12-381 -------------------------------------------------------------------------------------------------------------------
def words(v, n=12):
    return [(int(v) >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def wrows(vals, n=12):
    return np.array([words(v, n) for v in vals], dtype=U32)


def from_words(rows):
    return [sum(int(x) << (32 * i) for i, x in enumerate(r)) for r in rows]


def lrows(vals, n):
    return np.array([B.limbs(v, n) if isinstance(v, int) else v for v in vals], dtype=U32)


def host_rows(fn, op, a, b, width):
    out = np.zeros((len(a), width), U32)
    for i in range(len(a)):
        fn(op, ctypes.c_void_p(a[i].ctypes.data), ctypes.c_void_p(b[i].ctypes.data), ctypes.c_void_p(out[i].ctypes.data))
    return out


def binary(L, name, op, a, b, want, width):
    """one ds_bls_* entry of the (op, a, b, out) shape over a table: host == want, device == want under both masks"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    host = host_rows(getattr(L.hs, "hs_" + name), op, a, b, width)
    if want is not None:
        assert (host == want).all(), (name, op, first_bad(host == want, np.arange(len(a))))
    run_table(lambda t, o, m, n: dev(getattr(L.bls, "ds_" + name), op, t[0], t[1], o, m, n), [a, b], [("eq", host)], out_shape=(width,), out_dtype=U32, patterns=TWO)
    return host


def test_bls_field_ops_on_the_device(L):
    p, r, _ = O.bls_constants()
    vals = AC.bls_fp_values()
    a, b = wrows(vals[:-1]), wrows(vals[1:])
    for op, f in ((0, lambda x, y: x * y % p), (1, lambda x, y: (x + y) % p), (2, lambda x, y: (x - y) % p)):
        binary(L, "bls_fp_op", op, a, b, wrows([f(x, y) for x, y in zip(vals[:-1], vals[1:])]), 12)
    inv = binary(L, "bls_fp_op", 3, wrows(vals[1:12]), wrows([0] * 11), None, 12)
    assert all(x * y % p == 1 for x, y in zip(from_words(inv), vals[1:12]))
    binary(L, "bls_fp_op", 4, wrows(vals), wrows(vals), wrows([x * x % p for x in vals]), 12)
    # the scalar field
    vals, rng = AC.bls_fr_values()
    a, b = wrows(vals[:-1], 8), wrows(vals[1:], 8)
    for op, f in ((0, lambda x, y: x * y % r), (1, lambda x, y: (x + y) % r), (2, lambda x, y: (x - y) % r)):
        binary(L, "bls_fr_op", op, a, b, wrows([f(x, y) for x, y in zip(vals[:-1], vals[1:])], 8), 8)
    inv = binary(L, "bls_fr_op", 3, wrows(vals[1:10], 8), wrows([0] * 9, 8), None, 8)
    assert all(x * y % r == 1 for x, y in zip(from_words(inv), vals[1:10]))
    es = [int(rng.integers(0, 2**62)) for _ in vals[1:10]] + [0, 1, 2**64 - 1]
    base = vals[1:10] + [7, r - 1, r - 2]
    binary(L, "bls_fr_op", 4, wrows(base, 8), wrows(es, 8), wrows([pow(x, e, r) for x, e in zip(base, es)], 8), 8)
    # F_p^2
    pairs, _ = AC.bls_fp2_pairs()
    a = np.hstack([wrows([x[0][0] for x in pairs]), wrows([x[0][1] for x in pairs])])
    b = np.hstack([wrows([x[1][0] for x in pairs]), wrows([x[1][1] for x in pairs])])
    f2 = lambda c: np.hstack([wrows([v[0] for v in c]), wrows([v[1] for v in c])])
    binary(L, "bls_fp2_op", 0, a, b, f2([((x[0] * y[0] - x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p) for x, y in pairs]), 24)
    binary(L, "bls_fp2_op", 1, a, a, f2([((x[0] * x[0] - x[1] * x[1]) % p, 2 * x[0] * x[1] % p) for x, _ in pairs]), 24)
    inv = binary(L, "bls_fp2_op", 2, a, a, None, 24)
    for (x, _), row in zip(pairs, inv):
        i0, i1 = from_words([row[:12], row[12:]])
        assert ((x[0] * i0 - x[1] * i1) % p, (x[0] * i1 + x[1] * i0) % p) == (1, 0)


def test_bls_loose_primitives_on_the_device(L):
    """the loose (bounded, unreduced) arithmetic on raw limbs against the restatements of bls_rare_paths: the tables of
    test_bls_loose_field_primitives, the operands at the edge of the 64-bit column bound, lz_sub<K> / lz_weak<K> for every K"""
    p = B.P
    NL = B.FP_NL
    vals, rng = AC.bls_loose_values()
    rows = {0: [], 1: [], 2: [], 3: [], 4: []}
    for x in vals:
        for y in vals[::3]:
            if x * y < B.RADIX_P * p:
                rows[0].append((x, y))
            if x + y < B.RADIX_P:
                rows[1].append((x, y))
            if y <= 8 * p:
                rows[2].append((x, y))
        rows[3].append((x, 0))
        rows[4].append((x, 0))
    ref = {0: lambda x, y: B.value(B.lz_mul(B.limbs(x, NL), B.limbs(y, NL))), 1: lambda x, y: x + y, 2: lambda x, y: x + 8 * p - y,
           3: lambda x, y: x - 16 * p if x >= 16 * p else x, 4: lambda x, y: x % p}
    for op, pairs in rows.items():
        want = lrows([ref[op](x, y) for x, y in pairs], NL)
        got = binary(L, "bls_lz_op", op, lrows([x for x, _ in pairs], NL), lrows([y for _, y in pairs], NL), want, NL)
        if op == 0:
            assert all(B.value(g) < 2 * p and B.value(g) % p == x * y * B.RP_INV % p for g, (x, y) in zip(got, pairs))
    # the zero filter
    zs = [k * p for k in range(32)] + [B.rand_below(rng, 32 * p) for _ in range(600)]
    za = lrows(zs, NL)
    want = np.array([int(B.lz_maybe_zero(B.limbs(v, NL))) for v in zs], I32)
    assert want[:32].all() and (np.array([L.hs.hs_bls_lz_maybe_zero(ctypes.c_void_p(row.ctypes.data)) for row in za], I32) == want).all()
    run_table(lambda t, o, m, n: dev(L.bls.ds_bls_lz_maybe_zero, t[0], o, m, n), [za], [("eq", want)], out_dtype=I32, patterns=TWO)
    # raw limbs: columns at the edge of the 64-bit bound, unnormalised sums, saturated coordinates
    full = (B.LM,) * (NL - 1)
    ops = [full + (t,) for t in (0, 1, 0x1A010)]
    wide = [(1 << 29) - 1] * NL
    wide[-1] = (32 * p >> (B.LB * (NL - 1))) - 2
    ops.append(tuple(wide))
    ops += [B.limbs(B.mont_x(q), NL) for q in B.g1_saturated(4)]
    ops += [B.limbs(B.rand_below(rng, p), NL) for _ in range(12)]
    pairs = [(x, y) for x in ops for y in ops if B.value(x) * B.value(y) < B.RADIX_P * p]
    al, bl = lrows([x for x, _ in pairs], NL), lrows([y for _, y in pairs], NL)
    binary(L, "bls_fp_raw", 1, al, bl, lrows([B.lz_mul(x, y) for x, y in pairs], NL), NL)
    got = binary(L, "bls_fp_raw", 0, al, bl, None, NL)
    assert all(B.value(g) == B.value(x) * B.value(y) * B.RP_INV % p for g, (x, y) in zip(got, pairs))
    binary(L, "bls_fp_raw", 2, lrows(ops, NL), lrows(ops, NL), lrows([B.lz_sqr(x) for x in ops], NL), NL)
    canon = [B.limbs(B.rand_below(rng, p), NL) for _ in range(40)] + ops[:3]
    binary(L, "bls_fp_raw", 3, lrows(canon, NL), lrows(canon, NL), lrows([B.fp_mul(B.value(x), B.value(x)) for x in canon], NL), NL)
    sums = [(B.limbs(B.rand_below(rng, 32 * p), NL), B.limbs(B.rand_below(rng, 2 * p), NL)) for _ in range(100)]
    binary(L, "bls_fp_raw", 4, lrows([x for x, _ in sums], NL), lrows([y for _, y in sums], NL), lrows([B.lz_add_nc(x, y) for x, y in sums], NL), NL)
    # products of F_p that take the final subtraction (2^-11.3 each)
    found = []
    while len(found) < 20:
        x, y = B.rand_below(rng, p), B.rand_below(rng, p)
        if B.fp_t(x, y) >= p:
            found.append((x, y))
    binary(L, "bls_fp_raw", 0, lrows([x for x, _ in found], NL), lrows([y for _, y in found], NL), lrows([B.fp_t(x, y) - p for x, y in found], NL), NL)
    # lz_sub<K>, lz_weak<K>: K per element
    for weak in (0, 1):
        ks, xs, ys, want = [], [], [], []
        for K in (2, 4, 6, 8, 10, 12, 16, 18, 22):
            for j in range(40):
                if weak:
                    v = (B.rand_below(rng, 2 * K * p), K * p, K * p - 1, K * p + 1)[j % 4]
                    x = y = B.limbs(v, NL)
                    w = B.lz_weak(K, x)
                    assert w == B.limbs(v - K * p if v >= K * p else v, NL)
                else:
                    x, y = B.limbs(B.rand_below(rng, 22 * p), NL), B.limbs(B.rand_below(rng, K * p + 1), NL)
                    if j % 3 == 0:
                        x = B.lz_add_nc(x, B.limbs(B.rand_below(rng, 2 * p), NL))
                        y2 = B.limbs(B.rand_below(rng, K * p // 2), NL)
                        y = B.lz_add_nc(y2, y2)
                    w = B.lz_sub(K, x, y)
                    assert B.value(w) == B.value(x) + K * p - B.value(y)
                ks.append(K), xs.append(x), ys.append(y), want.append(w)
        ks, xs, ys, want = np.array(ks, I32), lrows(xs, NL), lrows(ys, NL), lrows(want, NL)
        host = np.zeros_like(want)
        for i in range(len(ks)):
            assert L.hs.hs_bls_lz_k(weak, int(ks[i]), ctypes.c_void_p(xs[i].ctypes.data), ctypes.c_void_p(ys[i].ctypes.data), ctypes.c_void_p(host[i].ctypes.data)) == 0
        assert (host == want).all()

        def launch(t, o, m, n):
            ret = np.full(int(n), -7, I32)
            dev(L.bls.ds_bls_lz_k, weak, t[0], t[1], t[2], o, ret, m, n)
            assert (ret[m != 0] == 0).all() and (ret[m == 0] == -7).all()
        run_table(launch, [ks, xs, ys], [("eq", want)], out_shape=(NL,), out_dtype=U32, patterns=TWO)


def test_bls_scalar_limbs_and_one_limb_product(L):
    rng = np.random.default_rng(4)
    NL, r = B.FR_NL, B.R
    pairs = [(B.rand_below(rng, r), B.rand_below(rng, r)) for _ in range(200)]
    planted = 0
    for y in [B.rand_below(rng, r) for _ in range(60)] + [r - 1, r - 2, B.R2_R, B.fr_mont(7)]:      # products that take the final subtraction
        x = B.plant_fr(y, rng)
        if x is not None:
            assert B.fr_subtracts(x, y)
            pairs.append((x, y))
            planted += 1
    assert planted >= 48
    pairs += [(x, y) for x in (0, 1, r - 1, r - 2, B.ONE_R, B.R2_R) for y in (0, 1, r - 1, B.ONE_R, B.R2_R)]
    al, bl = lrows([x for x, _ in pairs], NL), lrows([y for _, y in pairs], NL)
    binary(L, "bls_fr_raw", 0, al, bl, lrows([B.fr_mul(x, y) for x, y in pairs], NL), NL)
    binary(L, "bls_fr_raw", 1, al, bl, lrows([(x + y) % r for x, y in pairs], NL), NL)
    binary(L, "bls_fr_raw", 2, al, bl, lrows([(x - y) % r for x, y in pairs], NL), NL)
    loads = [B.plant_fr_load(rng) for _ in range(50)] + [0, 1, r - 1] + [B.rand_below(rng, r) for _ in range(50)]
    canon = np.zeros((len(loads), NL), U32)
    canon[:, :8] = wrows(loads, 8)
    binary(L, "bls_fr_raw", 3, canon, canon, lrows([x * B.RADIX_R % r for x in loads], NL), NL)
    # r1cs::mul_small
    sat = [B.value((B.LM,) * 9 + (t,)) for t in (0, 1, 0x73EC)] + [B.value((0,) * 9 + (0x73ED,)), r - (1 << 224), (r >> 224) << 224]
    ws = [0, 1, r - 1, r - 2] + [w for w in sat if w < r]
    grid = [(w, c) for w in ws for c in (2, 3, 1 << 27, (1 << 28) - 2, (1 << 28) - 1)]
    one_sub, near = B.mul_small_pairs(rng, 150)
    assert all(B.mul_small(w, c).n_sub == 1 for w, c in one_sub)
    grid += one_sub + near + [(r - 1 - B.rand_below(rng, 1 << int(rng.integers(1, 250))), (1 << 28) - 1 - B.rand_below(rng, 1 << int(rng.integers(1, 27)))) for _ in range(500)]
    w, c = lrows([g[0] for g in grid], NL), np.array([g[1] for g in grid], U32)
    want = lrows([g[0] * g[1] % r for g in grid], NL)
    host = np.zeros_like(want)
    for i in range(len(grid)):
        L.hs.hs_r1cs_mul_small(ctypes.c_void_p(w[i].ctypes.data), ctypes.c_uint32(int(c[i])), ctypes.c_void_p(host[i].ctypes.data))
    assert (host == want).all()
    run_table(lambda t, o, m, n: dev(L.bls.ds_r1cs_mul_small, t[0], t[1], o, m, n), [w, c], [("eq", want)], out_shape=(NL,), out_dtype=U32, patterns=TWO)


def flat(pt):
    """an affine point of G1 (x, y) or G2 ((x0, x1), (y0, y1)) as canonical words; None (infinity) as zeros"""
    return [w for xy in pt for c in (xy if isinstance(xy, tuple) else [xy]) for w in words(c)]


def unflat(row, two):
    v = from_words(np.asarray(row).reshape(-1, 12))
    return ((v[0], v[1]), (v[2], v[3])) if two else (v[0], v[1])


def group_table(L, two, rows):
    """rows: [(op, P or None, Q or None, k, expected point or None)] through ds_bls_g*_op and hs_bls_g*_op"""
    W2 = 48 if two else 24
    name = "bls_g2_op" if two else "bls_g1_op"
    zero = [0] * W2
    for op in sorted({r[0] for r in rows}):
        sel = [r for r in rows if r[0] == op]
        pxy = np.array([flat(r[1]) if r[1] else zero for r in sel], U32)
        qxy = np.array([flat(r[2]) if r[2] else zero for r in sel], U32)
        pinf, qinf = np.array([r[1] is None for r in sel], I32), np.array([r[2] is None for r in sel], I32)
        k = np.array([r[3] for r in sel], U32)
        want = np.array([flat(r[4]) if r[4] else zero for r in sel], U32)
        winf = np.array([r[4] is None for r in sel], I32)
        for i, r in enumerate(sel):
            out = np.zeros(W2, U32)
            inf = getattr(L.hs, "hs_" + name)(op, ptr(pxy[i].copy()), int(pinf[i]), ptr(qxy[i].copy()), int(qinf[i]), ctypes.c_uint32(int(k[i])), ptr(out))
            assert inf == winf[i] and (inf or (out == want[i]).all()), (name, op, i)

        def launch(t, o, m, n):
            ret = np.full(int(n), -7, I32)
            dev(getattr(L.bls, "ds_" + name), op, t[0], t[1], t[2], t[3], t[4], o, ret, m, n)
            on = m != 0
            assert (ret[on] == t[5][on]).all() and (ret[~on] == -7).all()
            o[on & (ret == 1)] = 0                # what the words hold for infinity is not specified
        run_table(launch, [pxy, pinf, qxy, qinf, k, winf], [("eq", want)], out_shape=(W2,), out_dtype=U32, patterns=TWO)


def test_bls_group_law_on_the_device(L):
    p, r, G = O.bls_constants()
    rows = []
    pts = AC.bls_g1_points()
    neg = lambda q: (q[0], p - q[1])
    for a in pts:
        for b in pts[:3]:
            rows += [(0, a, b, 0, O.bls_g1_add(a, b)), (1, a, b, 0, O.bls_g1_add(a, b))]
        dbl = O.bls_g1_mul(a, 2)
        rows += [(0, a, a, 0, dbl), (1, a, a, 0, dbl), (2, a, None, 0, dbl), (0, a, neg(a), 0, None), (1, a, neg(a), 0, None),
                 (0, a, None, 0, a), (0, None, a, 0, a), (1, None, a, 0, a)]
        rows += [(3, a, None, k, O.bls_g1_mul(a, k) if k else None) for k in AC.GROUP_SMALL_K]
    rows += [(2, None, None, 0, None), (3, None, None, 7, None)]
    group_table(L, False, rows)
    _, rng = AC.bls_fp2_pairs()
    pts = AC.bls_g2_points(rng)
    neg2 = lambda q: (q[0], ((-q[1][0]) % p, (-q[1][1]) % p))
    rows = []
    for a in pts:
        for b in pts[:2]:
            rows += [(0, a, b, 0, O.bls_g2_add(a, b)), (1, a, b, 0, O.bls_g2_add(a, b))]
        dbl = O.bls_g2_mul(a, 2)
        rows += [(0, a, a, 0, dbl), (1, a, a, 0, dbl), (2, a, None, 0, dbl), (0, a, neg2(a), 0, None), (1, a, neg2(a), 0, None), (0, a, None, 0, a), (0, None, a, 0, a)]
        rows += [(3, a, None, k, O.bls_g2_mul(a, k) if k else None) for k in (0, 1, 5, 65535)]
    group_table(L, True, rows)


def oracle_sum(points):
    add = O.bls_g2_add if isinstance(points[0][0], tuple) else O.bls_g1_add
    s = None
    for q in points:
        s = add(s, q)
    return s


def acc_words(acc):
    return [x for c in acc for f in B.components(c) for x in f]


def chains(L, two, lists):
    """bucket chains of one length each launch: the whole chain on the device (ds_bls_g*_chain), then step by step through
    ds_bls_g*_loose_step against the restatement (limbs and way) and out through ds_bls_g*_loose_out"""
    W2 = 48 if two else 24
    g = "g2" if two else "g1"
    for length in sorted({len(c) for c in lists}):
        sel = [c for c in lists if len(c) == length]
        xy = np.array([[w for q in c for w in flat(q)] for c in sel], U32)
        sums = [oracle_sum(c) for c in sel]
        want = np.array([flat(s) if s else [0] * W2 for s in sums], U32)
        winf = np.array([s is None for s in sums], I32)
        for i in range(len(sel)):
            out = np.zeros(W2, U32)
            inf = getattr(L.hs, "hs_bls_%s_chain" % g)(ptr(xy[i].copy()), ctypes.c_size_t(length), ptr(out))
            assert inf == winf[i] and (inf or (out == want[i]).all())

        def launch(t, o, m, n):
            ret = np.full(int(n), -7, I32)
            dev(getattr(L.bls, "ds_bls_%s_chain" % g), t[0], N(length), o, ret, m, n)
            on = m != 0
            assert (ret[on] == t[1][on]).all() and (ret[~on] == -7).all()
            o[on & (ret == 1)] = 0
        run_table(launch, [xy, winf], [("eq", want)], out_shape=(W2,), out_dtype=U32, patterns=TWO)
        # step by step
        accs = [B.xyzz_inf(two) for _ in sel]
        A = len(acc_words(accs[0]))
        for step in range(length):
            sts = [B.xyzz_add_mixed_loose(acc, B.mont_point(c[step])) for acc, c in zip(accs, sel)]
            a_in = np.array([acc_words(acc) for acc in accs], U32)
            q = np.array([flat(c[step]) for c in sel], U32)
            a_out = np.array([acc_words(st.acc) for st in sts], U32)
            ways = np.array([B.WAYS.index(st.way) for st in sts], I32)

            def launch(t, o, m, n):
                ret = np.full(int(n), -7, I32)
                dev(getattr(L.bls, "ds_bls_%s_loose_step" % g), t[0], t[1], o, ret, m, n)
                on = m != 0
                assert (ret[on] == t[2][on]).all() and (ret[~on] == -7).all()
            run_table(launch, [a_in, q, ways], [("eq", a_out)], out_shape=(A,), out_dtype=U32, patterns=TWO)
            accs = [st.acc for st in sts]
        a_in = np.array([acc_words(acc) for acc in accs], U32)

        def launch(t, o, m, n):
            ret = np.full(int(n), -7, I32)
            dev(getattr(L.bls, "ds_bls_%s_loose_out" % g), t[0], o, ret, m, n)
            on = m != 0
            assert (ret[on] == t[1][on]).all() and (ret[~on] == -7).all()
            o[on & (ret == 1)] = 0
        run_table(launch, [a_in, winf], [("eq", want)], out_shape=(W2,), out_dtype=U32, patterns=TWO)


def test_bls_bucket_accumulation_on_the_device(L):
    """xyzz_add_mixed_loose chained like k_bucket_sum does: random sums, the doubling branch, cancellation to infinity and on, false
    positives of the "same x?" filter in both orders, a family of pairwise false positives, saturated limbs"""
    p, r, G = O.bls_constants()
    G2 = O.bls_g2_generator()
    rng = np.random.default_rng(6)
    ks = AC.bls_bucket_scalars()
    g1 = [O.bls_g1_mul(G, k) for k in ks[:12]]
    a, b = g1[0], g1[1]
    nega = (a[0], p - a[1])
    lists = [g1, g1[:1], [a, a], [a, b, O.bls_g1_add(a, b), g1[2]], [a, nega], [a, nega, b, g1[3]]]
    for _ in range(3):
        x, y = B.g1_false_positive_pair(rng)
        lists += [[x, y], [y, x]]
    lists.append(B.g1_family(rng, 4))
    sat = B.g1_saturated(4)
    lists.append(sat + [B.random_g1(rng), sat[0]])
    chains(L, False, lists)
    g2 = [O.bls_g2_mul(G2, k) for k in ks[:6]]
    c, d = g2[0], g2[1]
    negc = (c[0], ((p - c[1][0]) % p, (p - c[1][1]) % p))
    lists = [g2, [c, c], [c, d, O.bls_g2_add(c, d), g2[2]], [c, negc], [c, negc, d, g2[3]]]
    for mode in ("both", "c0_zero", "c0_alias_c1_equal"):
        x, y = B.g2_false_positive_pair(rng, mode)
        lists += [[x, y], [y, x]]
    chains(L, True, lists)
