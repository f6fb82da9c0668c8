"""cp_fixed_base_mul_bls12381_g1_dev / _g2_dev against the oracle's scalar multiplication, point by point: sizes around a wave
and around the K = 4 results that share an inversion, the scalars the signed byte digits and the mixed addition can go wrong
on, another base and the table cache, the refusals, and the output form (an MSM over the produced set with the produced flags).
Everything is compared for equality. The refusal of an array on another device needs a second GPU and is not exercised here."""
import ctypes

import numpy as np
import pytest

import groth16_setup_cases as GC
import oracle_lib as O
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
R = GC.R
SIZES = (1, 63, 64, 65, 1000)     # partial waves (64 lanes x 4 scalars), partial groups of 4: 1, 63 and 65 are no multiples of 4


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


class Group:
    def __init__(self, name):
        import cityprover as cp
        self.name = name
        if name == "g1":
            self.points, self.gen, self.mul, self.add = cp.G1Points, O.bls_constants()[2], O.bls_g1_mul, O.bls_g1_add
            self.fn, self.words = "cp_fixed_base_mul_bls12381_g1_dev", 12
        else:
            self.points, self.gen, self.mul, self.add = cp.G2Points, O.bls_g2_generator(), O.bls_g2_mul, O.bls_g2_add
            self.fn, self.words = "cp_fixed_base_mul_bls12381_g2_dev", 24

    def base_words(self, base):
        coords = base if self.name == "g1" else (base[0][0], base[0][1], base[1][0], base[1][1])
        return np.array([(int(c) >> (64 * i)) & (2**64 - 1) for c in coords for i in range(6)], dtype=np.uint64)


@pytest.fixture(scope="module", params=["g1", "g2"])
def group(request):
    return Group(request.param)


def multiples(prover, group, base, scalars):
    """(points, flags) of the device call, on the host: points as the oracle writes them"""
    import cityprover as cp
    d = prover.to_device(RC.limbs4(scalars))
    try:
        pts, flags = group.points.fixed_base(prover, base, d.ptr, len(scalars))
        try:
            return pts.to_host(), cp.flags_to_host(flags, len(scalars))
        finally:
            pts.free()
            flags.free()
    finally:
        d.free()


def check(group, base, scalars, got):
    pts, flags = got
    for i, k in enumerate(scalars):
        want = group.mul(base, k)
        if want is None:
            assert flags[i] == 1, (i, hex(k))
            assert pts[i] == base, (i, hex(k))           # a valid point behind the flag: the base
        else:
            assert flags[i] == 0, (i, hex(k))
            assert pts[i] == want, (i, hex(k))


_random = {}


def random_reference(group):
    """1000 random 256-bit scalars and their multiples of the generator by the oracle: computed once per group"""
    if group.name not in _random:
        ks = GC.random_scalars(max(SIZES), 77)
        _random[group.name] = (ks, [group.mul(group.gen, k) for k in ks])
    return _random[group.name]


@pytest.mark.parametrize("n", SIZES)
def test_random_scalars_match_the_oracle(prover, group, n):
    ks, want = random_reference(group)
    pts, flags = multiples(prover, group, group.gen, ks[:n])
    assert not flags.any()
    assert pts == want[:n]


def test_edge_scalars(prover, group):
    ks = GC.edge_scalars()
    assert len(ks) > 40 and {0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1} <= set(ks)
    got = multiples(prover, group, group.gen, ks)
    check(group, group.gen, ks, got)
    assert got[1][ks.index(0)] == 1 and got[1][ks.index(R)] == 1 and got[1].sum() == 2
    # r - 1 is the negated base
    neg = got[0][ks.index(R - 1)]
    assert group.add(neg, group.gen) is None


def test_another_base_and_the_table_cache(prover, group):
    """a base other than the generator, then the generator on the same context (the cached table is replaced), then the first
    base again"""
    other = group.mul(group.gen, 0xC0FFEE1234567)
    ks = GC.random_scalars(70, 5) + [0, R - 1, R + 1]
    first = multiples(prover, group, other, ks)
    check(group, other, ks, first)
    check(group, group.gen, ks[:9], multiples(prover, group, group.gen, ks[:9]))
    assert multiples(prover, group, other, ks)[0] == first[0]


def test_refusals(prover, group):
    import cityprover as cp
    lib = prover.lib
    fn = getattr(lib, group.fn)
    g = group.base_words(group.gen)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    d = prover.to_device(RC.limbs4([1, 2, 3, 4]))
    out, flags = prover.alloc(4 * (14 if group.name == "g1" else 28)), prover.alloc(1)     # four points, four flags
    try:
        for args in ((None, d.ptr, 4, out.ptr, flags.ptr), (g.ctypes.data_as(u64p), None, 4, out.ptr, flags.ptr),
                     (g.ctypes.data_as(u64p), d.ptr, 4, None, flags.ptr), (g.ctypes.data_as(u64p), d.ptr, 4, out.ptr, None)):
            assert fn(prover.ctx, *args) == -1
            assert b"NULL" in lib.cp_last_error(prover.ctx)
        assert fn(prover.ctx, g.ctypes.data_as(u64p), d.ptr, 0, out.ptr, flags.ptr) == -1
        assert b"n = 0" in lib.cp_last_error(prover.ctx)
        bad = g.copy()
        bad[group.words // 2] ^= 1                    # y + 1 (or y - 1): off the curve
        assert fn(prover.ctx, bad.ctypes.data_as(u64p), d.ptr, 4, out.ptr, flags.ptr) == -1
        assert b"not on the curve" in lib.cp_last_error(prover.ctx)
        notcanon = g.copy()
        notcanon[:6] = 2**64 - 1                      # x >= p
        assert fn(prover.ctx, notcanon.ctypes.data_as(u64p), d.ptr, 4, out.ptr, flags.ptr) == -1
        assert b"canonical" in lib.cp_last_error(prover.ctx)
        assert fn(None, g.ctypes.data_as(u64p), d.ptr, 4, out.ptr, flags.ptr) == -1
        with pytest.raises(cp.CityProverError, match="n = 0"):
            group.points.fixed_base(prover, group.gen, d.ptr, 0)
        # the context is as usable as before
        check(group, group.gen, [1, 2, 3, 4], multiples(prover, group, group.gen, [1, 2, 3, 4]))
    finally:
        for b in (d, out, flags):
            b.free()


def test_an_msm_reads_the_produced_set_and_flags(prover, group):
    """sum_i s_i (k_i base) over the produced points with the produced flags = (sum_i s_i k_i) base: the output is in the form
    the MSMs read, and the entries flagged infinity are skipped"""
    ks = GC.edge_scalars()[:12] + GC.random_scalars(89, 9)          # 0 and r among them: two flagged entries
    ss = GC.random_scalars(len(ks), 10)
    dk, ds = prover.to_device(RC.limbs4(ks)), prover.to_device(RC.limbs4(ss))
    pts, flags = group.points.fixed_base(prover, group.gen, dk.ptr, len(ks))
    try:
        got = pts.msm_dev(ds.ptr, flags.ptr)
        assert got == group.mul(group.gen, sum(k * s for k, s in zip(ks, ss)) % R)
    finally:
        for b in (dk, ds, pts, flags):
            b.free()
