"""The paired forms behind the radix-16 NTT passes, checked on the CPU (a host build of their portable forms, tests/ntt_pairs_hostsim):
`gl::reduce128_lazy2` gives the very lazy words of two `gl::reduce128_lazy` and the values of Python integers on 128-bit words of
every class in slot A against every class in slot B (neither repairs, only A, only B, both; the fold wraps or not in each);
`reduce128_2` and `mul2` are their canonical forms; `ntt16::mul_pow2_2<Ka, Kb>` is two `mul_pow2` for every pair of shifts of one
form that `diff_times_w16` produces, in both directions. The operand arrays (tests/ntt_pair_cases.py) are the ones
tests/test_gpu_ntt_pairs.py feeds to the device. CPU only."""
import ctypes

import numpy as np
import pytest

import ntt_pair_cases as NP
import product_pairs as PP
import rare_paths as R

P = R.P
p64 = ctypes.POINTER(ctypes.c_uint64)


def ptr(x):
    return x.ctypes.data_as(p64)


def canon(x):
    return np.where(x >= np.uint64(P), x - np.uint64(P), x)


@pytest.fixture(scope="module")
def hs():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("ntt_pairs_hostsim"))
    lib.np_reduce2.argtypes = [p64] * 10 + [ctypes.c_size_t]
    lib.np_mul2.argtypes = [p64] * 8 + [ctypes.c_size_t]
    lib.np_pow2_2.argtypes = [ctypes.c_int, ctypes.c_int] + [p64] * 6 + [ctypes.c_size_t]
    lib.np_pow2_2.restype = ctypes.c_int
    return lib


def test_reduce_array_holds_every_combination_in_every_pattern():
    la, ha, lb, hb, _, _, blocks = NP.reduce_array()
    assert la.size == ha.size == lb.size == hb.size == len(blocks) * NP.N
    bA, wA = NP.reduce_classes(la, ha)
    bB, wB = NP.reduce_classes(lb, hb)
    for i in range(0, la.size, 997):       # the vectorised classes are the ones of rare_paths.reduce_paths
        pa = R.reduce_paths(int(la[i]), int(ha[i]))
        assert (pa.borrow, pa.fold_wrap) == (bool(bA[i]), bool(wA[i]))
    pats = R.patterns(NP.N)
    seen = {name: set() for name in R.PATTERNS}
    for ka, kb, name, off in blocks[:-1]:
        idx = off + np.nonzero(pats[name])[0]
        assert idx.size >= 8
        ra, rb = PP.repairs(ka), PP.repairs(kb)
        assert (bA[idx] == ra).all() and (bB[idx] == rb).all(), (ka, kb, name)   # the planted lanes repair as their class says
        for i in idx[:4]:
            seen[name].add((ra, bool(wA[i]), rb, bool(wB[i])))
    want = {(ra, wa, rb, wb) for ra in (False, True) for wa in (False, True) for rb in (False, True) for wb in (False, True)}
    for name in R.PATTERNS:
        assert seen[name] == want, (name, want - seen[name])


def test_portable_reduce128_lazy2_is_two_reduce128_lazy_and_python_integers(hs):
    la, ha, lb, hb, want_a, want_b, _ = NP.reduce_array()
    n = la.size
    r0, r1, s0, s1, c0, c1 = (np.zeros(n, np.uint64) for _ in range(6))
    hs.np_reduce2(ptr(la), ptr(ha), ptr(lb), ptr(hb), ptr(r0), ptr(r1), ptr(s0), ptr(s1), ptr(c0), ptr(c1), n)
    assert (r0 == s0).all() and (r1 == s1).all()           # the same lazy words, not only the same classes
    assert (canon(r0) == want_a).all() and (canon(r1) == want_b).all()
    assert (c0 == want_a).all() and (c1 == want_b).all()   # reduce128_2: canonical


def test_portable_mul2_is_two_mul_on_the_pair_array(hs):
    A, B, C_, D, _ = PP.pair_array()
    want_ab, want_cd = PP.pair_products()
    n = A.size
    r0, r1, s0, s1 = (np.zeros(n, np.uint64) for _ in range(4))
    hs.np_mul2(ptr(A), ptr(B), ptr(C_), ptr(D), ptr(r0), ptr(r1), ptr(s0), ptr(s1), n)
    assert (r0 == s0).all() and (r1 == s1).all()
    assert (r0 == want_ab).all() and (r1 == want_cd).all()


def test_shifts_are_the_ones_of_diff_times_w16_and_the_plan_pairs_one_form():
    assert NP.SHIFTS == [12, 24, 36, 48, 60, 72, 84]
    for inv in (False, True):
        for B in range(4):
            plan = NP.stage_plan(inv, B)
            regs = [r for ra, _, rb, _ in plan for r in (ra, rb) if r is not None]
            nontrivial = [m + (1 << B) for m in range(16) if not m & (1 << B) and R.W16_SHIFT[inv][(m & ((1 << B) - 1)) << (3 - B)] % 96]
            assert sorted(regs) == nontrivial                                    # every non-trivial shift once
            assert all(rb is None or NP.FORM(Ka) == NP.FORM(Kb) for _, Ka, rb, Kb in plan)
            assert sum(rb is None for _, _, rb, _ in plan) <= 2                  # at most one lone shift per form
        assert NP.first_stage_pair(inv, True)[1::2] in ((84, 72), (72, 84))


@pytest.mark.parametrize("inverse", [False, True])
def test_portable_mul_pow2_2_is_two_mul_pow2_for_every_pair_of_shifts(hs, inverse):
    """every ordered pair of shifts of one form (the plan's own pairs among them); `inverse` only changes which operands are drawn"""
    pairs = [(a, b) for a in NP.SHIFTS for b in NP.SHIFTS if NP.FORM(a) == NP.FORM(b)]
    planned = {(Ka, Kb) for B in range(4) for _, Ka, rb, Kb in NP.stage_plan(inverse, B) if rb is not None}
    assert planned <= set(pairs) and len(planned) >= 4
    for Ka, Kb in pairs:
        x, y, seen = NP.pow2_pair_operands(Ka, Kb, seed=int(inverse))
        reach = {(ra, rb) for ra, rb in NP.COMBOS if (not ra or Ka >= 33) and (not rb or Kb >= 33)}
        assert seen == reach, (Ka, Kb)
        n = x.size
        px, py, sx, sy = (np.zeros(n, np.uint64) for _ in range(4))
        assert hs.np_pow2_2(Ka, Kb, ptr(x), ptr(y), ptr(px), ptr(py), ptr(sx), ptr(sy), n) == 0
        assert (px == sx).all() and (py == sy).all(), (Ka, Kb)
        assert px.tolist() == [(v << Ka) % P for v in x.tolist()] and py.tolist() == [(v << Kb) % P for v in y.tolist()], (Ka, Kb)
    assert hs.np_pow2_2(12, 72, ptr(x), ptr(y), ptr(px), ptr(py), ptr(sx), ptr(sy), 0) == -1


def test_pair_inputs_put_the_repair_on_the_first_chain_the_second_and_both():
    for inv in (False, True):
        for combo in NP.COMBOS:
            x, wit = NP.ntt16_pair_input(12, inv, combo, R.patterns(256)["alternate"], 5)
            assert len(wit) == 128 and (x < np.uint64(P)).all()
            for da, Ka, db, Kb in wit[:16]:
                assert (R.pow2_paths(da, Ka).borrow, R.pow2_paths(db, Kb).borrow) == combo and Ka >= 64 and Kb >= 64
