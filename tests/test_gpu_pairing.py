"""cp_pairing_product_bls12381 on the device against tests/pairing_ref.py: every expected GT value is a power of the
reference's e(G1, G2)^c, computed once; every point is a known multiple of a generator made by the oracle. A pairing that is
wrong by a constant power or a missing conjugation passes every bilinearity check and fails the value comparisons here."""
import ctypes

import numpy as np
import pytest

import pairing_cases as PC
import pairing_ref as PR

pytestmark = pytest.mark.gpu
P, R = PR.P, PR.R
C = 3                       # the power the header states
N = 130
EDGE = (0, 63, 64, N - 1)   # wave and workgroup boundaries


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def batch():
    """130 pairs (a_i G1, b_i G2), distinct small and full-width a_i, b_i, and e(G1, G2)^(c a_i b_i)"""
    a, b = PC.scalars(N, 1), PC.scalars(N, 2)[::-1]
    g1 = np.stack([PC.g1_words(PC.g1_mul(k)) for k in a])
    g2 = np.stack([PC.g2_words(PC.g2_mul(k)) for k in b])
    gt = np.stack([PC.gt_words(PR.gt_power(C, x * y)) for x, y in zip(a, b)])
    for arr in (g1, g2, gt):
        arr.setflags(write=False)
    return {"a": a, "b": b, "g1": g1, "g2": g2, "gt": gt}


ONE = PC.gt_words(PR.F12_ONE)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gt_values_are_the_reference_values(prover, batch, n):
    import cityprover as cp
    gt, is_one, status = cp.pairing_product(prover, batch["g1"][:n], batch["g2"][:n])
    assert (status == 0).all() and (is_one == 0).all()
    assert gt.tobytes() == batch["gt"][:n].tobytes()


@pytest.mark.parametrize("k,n,one_row", [(2, 66, 64), (3, 5, 2), (4, 5, 0)])
def test_products_and_the_row_that_multiplies_to_one(prover, k, n, one_row):
    import cityprover as cp
    sc = PC.scalars(2 * n * k, 10 + k)
    g1, g2, want = [], [], []
    for row in range(n):
        logs = [(sc[2 * (row * k + j)], sc[2 * (row * k + j) + 1]) for j in range(k)]
        if row == one_row:   # (a G1, b G2), ..., (-(sum a b) G1, G2)
            logs[-1] = (-sum(x * y for x, y in logs[:-1]) % R, 1)
        g1 += [PC.g1_words(PC.g1_mul(x)) for x, _ in logs]
        g2 += [PC.g2_words(PC.g2_mul(y)) for _, y in logs]
        want.append(PC.gt_words(PR.gt_power(C, sum(x * y for x, y in logs))))
    assert want[one_row].tobytes() == ONE.tobytes()
    gt, is_one, status = cp.pairing_product(prover, np.stack(g1), np.stack(g2), k=k)
    assert (status == 0).all()
    assert is_one.tolist() == [int(row == one_row) for row in range(n)]
    assert gt.tobytes() == np.stack(want).tobytes()
    # the flag alone, without the values
    gt2, is_one2, _ = cp.pairing_product(prover, np.stack(g1), np.stack(g2), k=k, want_gt=False)
    assert gt2 is None and is_one2.tolist() == is_one.tolist()


def test_infinity_flags_give_the_identity(prover, batch):
    import cityprover as cp
    n = 66
    g1, g2 = batch["g1"][:n].copy(), batch["g2"][:n].copy()
    f1, f2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    f1[[0, 63]] = 1
    f2[[64, 65]] = 1
    f1[10] = f2[10] = 1
    g1[0] = 0                    # what a flagged entry holds is not looked at: zeros, a value >= p
    g1[63] = 2**64 - 1
    g2[64] = 2**64 - 1
    flagged = sorted({0, 10, 63, 64, 65})
    gt, is_one, status = cp.pairing_product(prover, g1, g2, g1_inf=f1, g2_inf=f2)
    want = batch["gt"][:n].copy()
    want[flagged] = ONE
    assert (status == 0).all()
    assert is_one.tolist() == [int(i in flagged) for i in range(n)]
    assert gt.tobytes() == want.tobytes()
    # inside a product the flagged pair is the neutral factor: rows of two pairs, the second flagged
    gt, is_one, status = cp.pairing_product(prover, batch["g1"][:4], batch["g2"][:4], k=2, g2_inf=np.array([0, 1, 0, 1], np.uint8))
    assert (status == 0).all() and (is_one == 0).all()
    assert gt.tobytes() == batch["gt"][[0, 2]].tobytes()


def test_trusted_gives_the_same_bytes(prover, batch):
    import cityprover as cp
    checked = cp.pairing_product(prover, batch["g1"], batch["g2"])
    trusted = cp.pairing_product(prover, batch["g1"], batch["g2"], flags=cp.PAIRING_TRUSTED)
    for x, y in zip(checked, trusted):
        assert x.tobytes() == y.tobytes()
    assert checked[0].tobytes() == batch["gt"].tobytes()


def _bad(kind, batch, i):
    """(g1 words, g2 words, status) of the bad pair that replaces pair i"""
    g1, g2 = batch["g1"][i].copy(), batch["g2"][i].copy()
    if kind == "g1_coordinate_p":
        g1[0:6] = PC.w6(P)
        return g1, g2, 1
    if kind == "g2_coordinate_p":
        g2[18:24] = PC.w6(P)
        return g1, g2, 1
    if kind == "g1_off_curve":
        g1[6] ^= 1
        return g1, g2, 2
    if kind == "g2_off_twist":
        g2[0] ^= 1
        return g1, g2, 2
    if kind == "g1_outside_torsion":
        return PC.g1_words(PC.g1_outside_torsion()), g2, 3
    assert kind == "g2_outside_torsion"
    return g1, PC.g2_words(PC.g2_outside_torsion()), 3


@pytest.mark.parametrize("kind", ["g1_coordinate_p", "g2_coordinate_p", "g1_off_curve", "g2_off_twist", "g1_outside_torsion", "g2_outside_torsion"])
def test_bad_points_are_verdicts_on_their_items(prover, batch, kind):
    import cityprover as cp
    g1, g2 = batch["g1"].copy(), batch["g2"].copy()
    want_gt, want_status = batch["gt"].copy(), np.zeros(N, np.uint8)
    for i in EDGE:
        g1[i], g2[i], want_status[i] = _bad(kind, batch, i)
        want_gt[i] = 0
    gt, is_one, status = cp.pairing_product(prover, g1, g2)
    assert status.tolist() == want_status.tolist()
    assert (is_one == 0).all()
    assert gt.tobytes() == want_gt.tobytes()
    if kind.endswith("outside_torsion"):   # trusted: no subgroup check, the item's value is unspecified, every other item is right
        gt, is_one, status = cp.pairing_product(prover, g1, g2, flags=cp.PAIRING_TRUSTED)
        assert (status == 0).all()
        keep = [i for i in range(N) if i not in EDGE]
        assert gt[keep].tobytes() == batch["gt"][keep].tobytes()


def test_a_bad_pair_spoils_its_whole_product_and_no_other(prover, batch):
    import cityprover as cp
    g1, g2 = batch["g1"][:6].copy(), batch["g2"][:6].copy()
    g1[3], g2[3], _ = _bad("g1_off_curve", batch, 3)
    g1[2], g2[2], _ = _bad("g2_outside_torsion", batch, 2)      # the first bad pair of the row decides: pair 2 comes before pair 3
    gt, is_one, status = cp.pairing_product(prover, g1, g2, k=2)
    assert status.tolist() == [0, 3, 0] and (is_one == 0).all()
    a, b = batch["a"], batch["b"]
    want = [PC.gt_words(PR.gt_power(C, a[0] * b[0] + a[1] * b[1])), np.zeros(72, np.uint64), PC.gt_words(PR.gt_power(C, a[4] * b[4] + a[5] * b[5]))]
    assert gt.tobytes() == np.stack(want).tobytes()


def test_argument_refusals_leave_the_context_usable(prover, batch):
    import cityprover as cp
    lib = prover.lib
    u64p, u8p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    g1, g2 = batch["g1"][:2].copy(), batch["g2"][:2].copy()
    gt, flag = np.full((2, 72), 9, np.uint64), np.full(2, 9, np.uint8)
    p1, p2, pg, pf = g1.ctypes.data_as(u64p), g2.ctypes.data_as(u64p), gt.ctypes.data_as(u64p), flag.ctypes.data_as(u8p)
    INVALID = -1
    calls = [((None, None, p2, None, 2, 1, 0, pg, pf, None), "NULL point array"), ((p1, None, None, None, 2, 1, 0, pg, pf, None), "NULL point array"),
             ((p1, None, p2, None, 0, 1, 0, pg, pf, None), "at least 1"), ((p1, None, p2, None, 2, 0, 0, pg, pf, None), "at least 1"),
             ((p1, None, p2, None, 2, 1, 0, None, None, None), "both outputs are NULL"), ((p1, None, p2, None, 2, 1, 2, pg, pf, None), "unknown flag")]
    for args, msg in calls:
        assert lib.cp_pairing_product_bls12381(prover.ctx, *args) == INVALID, msg
        assert msg.encode() in lib.cp_last_error(prover.ctx), msg
        assert (gt == 9).all() and (flag == 9).all()
        out, _, status = cp.pairing_product(prover, g1, g2)        # the same context, straight afterwards
        assert (status == 0).all() and out.tobytes() == batch["gt"][:2].tobytes()
