"""Every NTT / LDE launch form pinned to the CPU oracle, and proven from the profile to have run.

The DIF planner (cityprover.hip run_dif) cuts a transform into passes of L bits: below 2^12 one pass of the generic kernel
(ntt.h), from 2^12 register radix-16 passes (ntt16.h) whose plan is 13 -> 7+6, 16..20 -> L+12, 21 -> 7+7+7, 24 -> 8+4+12. Around
it: the natural-order LDS epilogue at 2^12, the bit-reversal copy, the staged store of the last pass from 2^16
(CITYPROVER_NTT_STAGED_STORE), the LDE as 2^rate coset transforms at 2^12 with a pre-scale table, the zero-padded LDE elsewhere,
and the generic kernel at >= 2^12 under CITYPROVER_NTT_V1. `ntt_plan` restates the planner; every case asserts the launches it
predicts. The GPU is touched only inside tests."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_TILE = 12           # ntt.h LOG_TILE_MAX == ntt16.h LOG_TILE
INVERSE, BITREV_OUT, COSET = 1, 2, 4   # cityprover.NTT_*
EDGE = np.array([0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFE00000002, 1 << 63, P >> 1, 7],
                dtype=np.uint64)
LABELS = ("ntt16_rows", "ntt16_cols", "ntt_dif_pass_rows", "ntt_dif_pass_cols", "ntt_bitrev_copy", "lde_pad_copy")

# switch -> the tests of this module that set it (tests/test_switch_coverage.py)
FORMS = {"NTT_STAGED_STORE": ["test_ntt_without_staged_store_matches_oracle"]}


def dif_plan(log_n, need16=False, v1=False):
    """[(L, label)] of run_dif's passes"""
    out, q = [], log_n
    while q > 0:
        if q <= LOG_TILE:
            L = q
        else:
            front = q - LOG_TILE
            if 4 <= front <= LOG_TILE - 4:
                L = front
            else:
                passes = (q + 9) // 10
                L = (q + passes - 1) // passes
        q_after = q - L
        c = min(LOG_TILE - L, log_n - L)
        if q_after > 0:
            c = min(c, q_after)
        kind = "rows" if q_after == 0 else "cols"
        radix16 = L >= 4 and L + c == LOG_TILE and (need16 or not v1)
        out.append((L, ("ntt16_" if radix16 else "ntt_dif_pass_") + kind))
        q = q_after
    return out


def ntt_plan(log_n, flags, v1=False):
    """launch label -> count of one cp_ntt_dev call"""
    coset, inverse = bool(flags & COSET), bool(flags & INVERSE)
    got = collections.Counter()
    natural12 = log_n == LOG_TILE and not flags & BITREV_OUT and not (coset and inverse)
    for _, label in dif_plan(log_n, need16=natural12, v1=v1):
        got[label] += 1
    if not flags & BITREV_OUT and not natural12:
        got["ntt_bitrev_copy"] += 1
    return got


def lde_plan(log_n, rate, bitrev):
    if log_n == LOG_TILE and bitrev and rate <= 6:
        return collections.Counter({"ntt16_rows": 1})   # one workgroup-resident pass per coset block (grid.z)
    got = ntt_plan(log_n + rate, (BITREV_OUT if bitrev else 0) | COSET)
    got["lde_pad_copy"] += 1
    return got


def test_planner_matches_the_documented_plans():
    """CPU only: the restated planner gives the pass plans the kernels were written for"""
    Ls = lambda log_n: [L for L, _ in dif_plan(log_n)]
    assert Ls(13) == [7, 6] and Ls(21) == [7, 7, 7] and Ls(24) == [8, 4, 12]
    assert all(Ls(n) == [n - 12, 12] for n in range(16, 21))
    assert all(dif_plan(n) == [(n, "ntt_dif_pass_rows")] for n in range(1, 12))
    assert dif_plan(24) == [(8, "ntt16_cols"), (4, "ntt16_cols"), (12, "ntt16_rows")]
    assert {lab for _, lab in dif_plan(17, v1=True)} == {"ntt_dif_pass_cols", "ntt_dif_pass_rows"}


def measured(prover, fn):
    prover.profile_begin()
    try:
        fn()
    finally:
        prof = prover.profile_end()
    return collections.Counter({k: v["launches"] for k, v in prof.items() if k in LABELS})


def call(prover, fn, *args, **kw):
    box = {}
    launches = measured(prover, lambda: box.update(r=fn(*args, **kw)))
    return box["r"], launches


def felts(n, seed):
    return O.splitmix64_felts(0x7E57 + seed, n)


def batch_for(log_n):
    return 3 if log_n <= 18 else 2 if log_n <= 22 else 1


def inputs(log_n):
    n, b = 1 << log_n, batch_for(log_n)
    x = felts(n * b, log_n).reshape(b, n)
    k = min(n, EDGE.size)
    x[0, :k] = EDGE[:k]
    x[-1, n - k:] = EDGE[:k]
    return x


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def check_all_forms(p, log_n, v1=False):
    """forward, inverse, bit-reversed forward, coset forward + inverse: every row against the oracle, launches as planned"""
    x = inputs(log_n)
    fwd = [O.ntt(r) for r in x]
    cases = [(0, x, fwd), (INVERSE, x, [O.intt(r) for r in x]), (BITREV_OUT, x, [O.bit_reverse(f) for f in fwd])]
    cos = [O.coset_lde(r, 0, 7) for r in x]
    cases += [(COSET, x, cos), (COSET | INVERSE, np.stack(cos), list(x))]
    for flags, inp, want in cases:
        got, launches = call(p, p.ntt, inp, flags=flags, shift=7 if flags & COSET else 0)
        for b in range(inp.shape[0]):
            assert (got[b] == want[b]).all(), (log_n, flags, b)
        assert launches == ntt_plan(log_n, flags, v1), (log_n, flags, dict(launches))


@pytest.mark.parametrize("log_n", range(1, 25))
def test_lone_transforms_match_oracle_with_planned_launches(prover, log_n):
    check_all_forms(prover, log_n)


def test_ntt_without_staged_store_matches_oracle():
    import cityprover
    p = cityprover.Prover(0)
    try:
        p.set_option("NTT_STAGED_STORE", 0)
        for log_n in range(16, 25):
            x = inputs(log_n)
            for flags in (0, INVERSE, BITREV_OUT):
                got, launches = call(p, p.ntt, x, flags=flags)
                for b in range(x.shape[0]):
                    want = O.intt(x[b]) if flags & INVERSE else O.ntt(x[b])
                    assert (got[b] == (O.bit_reverse(want) if flags & BITREV_OUT else want)).all(), (log_n, flags, b)
                assert launches == ntt_plan(log_n, flags), (log_n, flags)
    finally:
        p.close()


@pytest.mark.parametrize("log_n,batch,flags", [(12, 3, 0), (12, 2, INVERSE), (17, 3, 0), (17, 2, BITREV_OUT), (21, 2, 0)])
def test_strided_batches_leave_the_gaps_alone(prover, log_n, batch, flags):
    n = 1 << log_n
    stride = n + 40
    host = felts(stride * batch, 100 + log_n + flags)
    buf = prover.to_device(host)
    try:
        launches = measured(prover, lambda: prover.ntt_dev(buf.ptr, log_n, batch, stride, flags))
        out = buf.download()
    finally:
        buf.free()
    for b in range(batch):
        row = host[b * stride:b * stride + n]
        want = O.intt(row) if flags & INVERSE else O.ntt(row)
        assert (out[b * stride:b * stride + n] == (O.bit_reverse(want) if flags & BITREV_OUT else want)).all(), (log_n, b)
        assert (out[b * stride + n:(b + 1) * stride] == host[b * stride + n:(b + 1) * stride]).all(), ("gap", log_n, b)
    assert launches == ntt_plan(log_n, flags)


@pytest.mark.parametrize("rate", range(7))
def test_prescaled_lde_at_4096_with_strides(prover, rate):
    """2^rate coset transforms of 4096 points reading the coefficients once (cp_lde_dev pre-scale path), strided both sides"""
    log_n, batch = 12, 2
    n = 1 << log_n
    N = n << rate
    in_stride, out_stride = n + 24, N + 56
    coeffs = felts(in_stride * batch, 200 + rate)
    sentinel = felts(out_stride * batch, 300 + rate)
    for shift in (7, 3):
        din, dout = prover.to_device(coeffs), prover.to_device(sentinel)
        try:
            launches = measured(prover, lambda: prover.lde_dev(din.ptr, log_n, rate, batch, dout.ptr, shift=shift,
                                                               in_stride=in_stride, out_stride=out_stride))
            out = dout.download()
            assert (din.download() == coeffs).all()
        finally:
            din.free()
            dout.free()
        for b in range(batch):
            want = O.bit_reverse(O.coset_lde(coeffs[b * in_stride:b * in_stride + n], rate, shift))
            assert (out[b * out_stride:b * out_stride + N] == want).all(), (rate, shift, b)
            assert (out[b * out_stride + N:(b + 1) * out_stride] == sentinel[b * out_stride + N:(b + 1) * out_stride]).all(), ("gap", rate, b)
        assert launches == lde_plan(log_n, rate, True), (rate, shift, dict(launches))


@pytest.mark.parametrize("log_n", [10, 13, 16])
@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("bitrev", [False, True])
def test_padded_lde_matches_oracle(prover, log_n, rate, bitrev):
    n = 1 << log_n
    c = felts(2 * n, 400 + log_n + rate).reshape(2, n)
    c[0, :EDGE.size] = EDGE
    got, launches = call(prover, prover.lde, c, rate, shift=7, bitrev=bitrev)
    for b in range(2):
        want = O.coset_lde(c[b], rate, 7)
        assert (got[b] == (O.bit_reverse(want) if bitrev else want)).all(), (log_n, rate, bitrev, b)
    assert launches == lde_plan(log_n, rate, bitrev), dict(launches)


def legacy_generic_kernel_checks(prover):
    """the body of test_legacy_generic_kernel_at_4096_and_up: runs in a process started with CITYPROVER_NTT_V1 set"""
    for log_n in range(13, 18):
        x = inputs(log_n)
        for flags in (0, INVERSE):
            got, launches = call(prover, prover.ntt, x, flags=flags)
            for b in range(x.shape[0]):
                assert (got[b] == (O.intt(x[b]) if flags & INVERSE else O.ntt(x[b]))).all(), (log_n, flags, b)
            assert launches == ntt_plan(log_n, flags, v1=True), (log_n, flags, dict(launches))
            assert not launches["ntt16_rows"] and not launches["ntt16_cols"]
    x = inputs(12)
    got, launches = call(prover, prover.ntt, x, flags=BITREV_OUT)
    for b in range(x.shape[0]):
        assert (got[b] == O.bit_reverse(O.ntt(x[b]))).all(), b
    assert launches == {"ntt_dif_pass_rows": 1}
    # the natural-order epilogue at 2^12 needs the radix-16 kernel whatever the switch says
    got, launches = call(prover, prover.ntt, x)
    assert (got[0] == O.ntt(x[0])).all()
    assert launches == {"ntt16_rows": 1}


CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import cityprover
import test_gpu_ntt_forms as T
p = cityprover.Prover(0)
T.legacy_generic_kernel_checks(p)
p.close()
print("ntt v1 ok")
"""


def test_legacy_generic_kernel_at_4096_and_up():
    """CITYPROVER_NTT_V1 (read once per process, a function-static): the generic kernel instead of radix-16 wherever the caller
    does not need the latter, in a fresh child"""
    env = dict(os.environ, CITYPROVER_NTT_V1="1")
    code = CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "city-rollup_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0 and "ntt v1 ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
