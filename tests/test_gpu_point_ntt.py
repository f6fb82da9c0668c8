"""cp_point_ntt_bls12381_g1_dev / _g2_dev against the F_r transform in the exponent: the points [e_k] G go in, and the output
must be [fr_ntt(e)_j] G at every index - the transformed exponents by the oracle, their multiples by the fixed-base multiplication
(tests/test_gpu_fixed_base.py pins it), compared as points through to_host and as raw device bytes (the form the MSMs read:
reduced Montgomery limbs, the generator under an infinity flag). Degenerate inputs reach every branch of the complete addition
inside a butterfly: P = Q, P = -Q, either operand at infinity. Everything is compared for equality."""
import numpy as np
import pytest

import groth16_setup_cases as GC
import oracle_lib as O
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
R = GC.R
NTT_COSET = 4


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
            self.points, self.gen, self.mul, self.ntt = cp.G1Points, O.bls_constants()[2], O.bls_g1_mul, cp.point_ntt_g1_dev
        else:
            self.points, self.gen, self.mul, self.ntt = cp.G2Points, O.bls_g2_generator(), O.bls_g2_mul, cp.point_ntt_g2_dev


@pytest.fixture(scope="module", params=["g1", "g2"])
def group(request):
    return Group(request.param)


def exponent_points(prover, group, e):
    """(points, flags) on the device: [e_k] G, flagged infinity (the entry is G) where e_k = 0"""
    d = prover.to_device(RC.limbs4(e))
    try:
        return group.points.fixed_base(prover, group.gen, d.ptr, len(e))
    finally:
        d.free()


def snapshot(prover, pts, flags, n):
    import cityprover as cp
    prover.sync()
    return pts.buf.download().tobytes(), cp.flags_to_host(flags, n).tolist(), pts.to_host()


def transformed(e, inverse):
    return [int(v) for v in RC.from_limbs4(O.fr_ntt(RC.limbs4(e), inverse=inverse))]


def run_case(prover, group, e, inverse, oracle_points=False):
    """transform [e_k] G on the device and hold every output against [fr_ntt(e)_j] G"""
    n = len(e)
    log_n = n.bit_length() - 1
    want_e = transformed(e, inverse)
    pts, flags = exponent_points(prover, group, e)
    ref, ref_flags = exponent_points(prover, group, want_e)
    try:
        group.ntt(prover, pts, flags, log_n, inverse=inverse)
        got_bytes, got_flags, got = snapshot(prover, pts, flags, n)
        want_bytes, want_flags, want = snapshot(prover, ref, ref_flags, n)
        assert want_flags == [int(x == 0) for x in want_e]
        assert got_flags == want_flags                     # set exactly where the transformed exponent is 0
        assert got == want
        assert got_bytes == want_bytes                     # and the same device form, the generator under a flag included
        if oracle_points:                                  # the small sizes also against the oracle's own multiplication
            assert got == [group.mul(group.gen, x) if x else group.gen for x in want_e]
    finally:
        for b in (pts.buf, flags, ref.buf, ref_flags):
            b.free()


def seeded(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 5, 6, 9])
def test_against_the_transform_of_the_exponents(prover, group, log_n, inverse):
    """2^9 points are more than one workgroup of butterflies (256 > 128 / 64 lanes) and more than one wave of finishing lanes"""
    run_case(prover, group, seeded(1 << log_n, 1000 + log_n), inverse, oracle_points=log_n <= 3)


def test_inverse_after_forward_restores_the_input_bytes(prover, group):
    n = 32
    pts, flags = exponent_points(prover, group, seeded(n, 55))
    try:
        before = snapshot(prover, pts, flags, n)
        group.ntt(prover, pts, flags, 5)
        middle = snapshot(prover, pts, flags, n)
        group.ntt(prover, pts, flags, 5, inverse=True)
        assert middle[0] != before[0]
        assert snapshot(prover, pts, flags, n) == before
    finally:
        pts.buf.free()
        flags.free()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("kind", ["all_equal", "one_then_infinity", "alternating_sign", "all_infinity"])
def test_degenerate_inputs_reach_every_branch_of_the_addition(prover, group, kind, log_n, inverse):
    n = 1 << log_n
    e0 = seeded(1, 77)[0]
    e = {"all_equal": [e0] * n,                       # every first-stage butterfly adds P to P and subtracts P from P
         "one_then_infinity": [1] + [0] * (n - 1),    # the zeros are flagged-infinity entries: infinity on either side
         "alternating_sign": [1 if k % 2 == 0 else R - 1 for k in range(n)],   # P and -P across the stages
         "all_infinity": [0] * n}[kind]
    if kind == "all_equal" and not inverse:
        assert transformed(e, False) == [n * e0 % R] + [0] * (n - 1)
    run_case(prover, group, e, inverse, oracle_points=True)


def test_refusals_leave_the_context_usable(prover, group):
    import cityprover as cp
    pts, flags = exponent_points(prover, group, seeded(8, 5))
    try:
        before = snapshot(prover, pts, flags, 8)
        for kw, msg in (({"log_n": 29}, "log_n 29 out of range"), ({"log_n": -1}, "log_n -1 out of range"),
                        ({"log_n": 3, "flags": NTT_COSET}, "unsupported flags 0x4"), ({"log_n": 3, "flags": 1 | NTT_COSET}, "unsupported flags 0x5"),
                        ({"log_n": 3, "flags": 0x80}, "unsupported flags 0x80")):
            with pytest.raises(cp.CityProverError, match=msg):
                group.ntt(prover, pts, flags, **kw)
        with pytest.raises(cp.CityProverError, match="NULL argument"):
            group.ntt(prover, None, flags, 3)
        with pytest.raises(cp.CityProverError, match="NULL argument"):
            group.ntt(prover, pts, None, 3)
        assert snapshot(prover, pts, flags, 8) == before   # nothing was touched
    finally:
        pts.buf.free()
        flags.free()
    run_case(prover, group, seeded(1, 1000), False, oracle_points=True)   # the first case again, on the same context
