"""Operands for the paired forms the radix-16 NTT passes are built from (csrc/gl.h `reduce128_lazy2`, `mul2`; csrc/ntt16.h
`mul_pow2_2`, `stage_pairs`): two chains issued alternately, their borrow masks ORed and tested once, both repaired behind that one
branch. What can go wrong in a pair and not in a single chain is the coupling, so every array here puts each class in slot A against
each class in slot B. Pure Python, no GPU; shared by tests/test_gl_reduce_pairs.py and tests/test_gpu_ntt_pairs.py."""
import numpy as np

import product_pairs as PP
import rare_paths as R

P, M64, EPS = R.P, R.M64, R.EPS
N = 512   # lanes kept of every (class pair, lane pattern) block of product_pairs.pair_array: two workgroups, every pattern still shows

# ---- the shifts of ntt16.h ------------------------------------------------------------------------------------------------------
SHIFTS = sorted({sh % 96 for inv in (False, True) for sh in R.W16_SHIFT[inv]} - {0})   # every K diff_times_w16 hands to mul_pow2
FORM = lambda K: K >= 64                                                                # the two forms of mul_pow2


def stage_plan(inverse, B):
    """ntt16.h `shift_plan<INV, B>` restated: [(reg_a, K_a, reg_b, K_b)] (reg_b None: a lone shift) for the stage at field bit B, the
    non-trivial shifts in register order, each pairing with the next one of its form"""
    plan, pend = [], {False: None, True: None}
    for m in range(16):
        if m & (1 << B):
            continue
        K = R.W16_SHIFT[inverse][(m & ((1 << B) - 1)) << (3 - B)] % 96
        if K == 0:
            continue
        reg = m + (1 << B)
        if pend[FORM(K)] is None:
            pend[FORM(K)] = (reg, K)
        else:
            plan.append(pend[FORM(K)] + (reg, K))
            pend[FORM(K)] = None
    for form in (False, True):
        if pend[form] is not None:
            plan.append(pend[form] + (None, None))
    return plan


# ---- 128-bit words for reduce128_lazy2 ------------------------------------------------------------------------------------------
_REDUCE = None


def reduce_array():
    """(lo_a, hi_a, lo_b, hi_b, want_a, want_b, blocks): the true 128-bit products of product_pairs.pair_array, the first N lanes of every
    block — slot A reduces a b, slot B c d — and after them one block of arbitrary words (no products: any lo, any hi, edges included).
    blocks: [(key_a, key_b, pattern, offset)]; want: the values mod p with Python integers. Computed once."""
    global _REDUCE
    if _REDUCE is None:
        A, B, C_, D, blocks = PP.pair_array()
        keep = np.concatenate([np.arange(off, off + N) for _, _, _, off, _ in blocks])
        rng = np.random.default_rng(77)
        edge = [0, 1, EPS - 1, EPS, EPS + 1, 1 << 32, P - 1, P, P + 1, M64 - 1, M64, 0xFFFFFFFF00000000, 1 << 63]
        cols = []
        for x, y in ((A, B), (C_, D)):
            prod = [a * b for a, b in zip(x[keep].tolist(), y[keep].tolist())]
            lo, hi = [v & M64 for v in prod], [v >> 64 for v in prod]
            extra_lo = rng.integers(0, 1 << 64, N, dtype=np.uint64).tolist()
            extra_hi = rng.integers(0, 1 << 64, N, dtype=np.uint64).tolist()
            for i, (e, f) in enumerate((e, f) for e in edge for f in edge):
                extra_lo[i], extra_hi[i] = (e, f) if x is A else (f, e)
            cols.append((lo + extra_lo, hi + extra_hi))
        want = [np.array([(l + (h << 64)) % P for l, h in zip(lo, hi)], dtype=np.uint64) for lo, hi in cols]
        arrs = [np.array(v, dtype=np.uint64) for c in cols for v in c]
        new_blocks = [(ka, kb, name, i * N) for i, (ka, kb, name, _, _) in enumerate(blocks)] + [("any", "any", "every_lane", len(blocks) * N)]
        _REDUCE = (arrs[0], arrs[1], arrs[2], arrs[3], want[0], want[1], new_blocks)
    return _REDUCE


def reduce_classes(lo, hi):
    """(borrow, fold wrap) of reduce128_lazy(lo, hi) per element, vectorised (rare_paths.reduce_paths with numpy words)"""
    w2, w3 = hi & np.uint64(EPS), hi >> np.uint64(32)
    borrow = lo < w3
    t0 = lo - w3 - np.where(borrow, np.uint64(EPS), np.uint64(0))
    s = t0 + w2 * np.uint64(EPS)
    return borrow, s < t0


# ---- operands for mul_pow2_2<K0, K1> --------------------------------------------------------------------------------------------
def quiet_operand(K, rng):
    """canonical d != 0 whose mul_pow2<K> does NOT take the borrow repair"""
    while True:
        if K < 64:
            d = int(rng.integers(1, P, dtype=np.uint64))          # a random word has a non-zero low word: no borrow
        else:
            d = int(rng.integers(1, 1 << (96 - K)))               # (d << (K - 64)) stays below 2^32: w3 == 0
        if not R.pow2_paths(d, K).borrow:
            return d


def pow2_operand(K, repairs, rng):
    """canonical d whose mul_pow2<K> takes the repair (None when no operand of this K can: K <= 32) or does not"""
    if not repairs:
        return quiet_operand(K, rng)
    return R.pow2_borrow_operand(K, rng) if K >= 33 else None


COMBOS = ((False, False), (True, False), (False, True), (True, True))   # (first chain repairs, second chain repairs)


def pow2_pair_operands(Ka, Kb, n=256, seed=0):
    """(x, y, combos): n operand pairs for mul_pow2_2<Ka, Kb>, cycling through COMBOS (those a shift cannot reach are skipped), with 0, 1
    and p - 1 at the end. combos: the set of COMBOS that occur."""
    rng = np.random.default_rng(1000 * Ka + Kb + seed)
    x, y, seen = [], [], set()
    for i in range(n):
        ra, rb = COMBOS[i % 4]
        a, b = pow2_operand(Ka, ra, rng), pow2_operand(Kb, rb, rng)
        if a is None or b is None:
            continue
        x.append(a)
        y.append(b)
        seen.add((ra, rb))
    for e in (0, 1, P - 1):
        for f in (0, 1, P - 1):
            x.append(e)
            y.append(f)
    return np.array(x, dtype=np.uint64), np.array(y, dtype=np.uint64), seen


# ---- transforms whose first-stage PAIR repairs in its first chain, its second, or both ------------------------------------------
def first_stage_pair(inverse, form):
    """the first pair of the first stage (field bit 3) whose shifts are in `form`: (E_a, K_a, E_b, K_b), E the twiddle exponent = the
    eighth of the first half the butterfly lies in"""
    for ra, Ka, rb, Kb in stage_plan(inverse, 3):
        if rb is not None and FORM(Ka) == form:
            return ra - 8, Ka, rb - 8, Kb
    raise AssertionError("no pair of that form")


def ntt16_pair_input(log_n, inverse, combo, mask, seed):
    """One polynomial for the register radix-16 kernels. The thread that owns index t < n/16 holds t + m n/16 (m = 0..15) and its first
    stage pairs m with m + 8: difference E is x[t + E n/16] - x[t + E n/16 + n/2] (or its negative, by the sign of the shift), shifted by
    K_E. For every t under the mask the two differences of the K >= 64 pair are chosen as `combo` = (first repairs, second repairs) says
    (the other half of each butterfly is 0, so the difference is the planted word). K >= 64 because there a random word repairs and a
    short one does not: the K < 64 pairs of the plan are (K >= 33, K <= 32), whose second chain cannot repair at all —
    rare_paths.ntt16_borrow_input with a mask over one eighth covers their (first only). Returns x, witnesses [(d_a, K_a, d_b, K_b)]."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    x = rng.integers(0, P, n, dtype=np.uint64)
    Ea, Ka, Eb, Kb = first_stage_pair(inverse, True)
    wit = []
    for t in np.nonzero(mask)[0]:
        ds = []
        for E, K, rep in ((Ea, Ka, combo[0]), (Eb, Kb, combo[1])):
            d = pow2_operand(K, rep, rng)
            j = int(t) + E * (n >> 4)
            neg = R.W16_SHIFT[inverse][E] >= 96
            x[j], x[j + n // 2] = (0, d) if neg else (d, 0)
            ds += [d, K]
        wit.append(tuple(ds))
    return x, wit
