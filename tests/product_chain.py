"""The carry-aware product chain of csrc/gl.h (`mul_wide_cy` + `reduce128_lazy(lo, hi', cy)` + `fold_top`) restated with Python
integers, its proof obligations as assertions, and the witness array that tests/test_gpu_product_chain.py feeds to the device.
Pure Python, no GPU.

A product falls into one of twelve classes (cy, low-word borrow, 64-bit borrow, fold wrap): the carry-out of the third
multiply-add, the borrow out of `lo0 - hi32(hi') - cy`, the borrow out of the whole 64-bit subtraction (it implies the first, hence
2 x 3 x 2 classes) and the wrap of the final `+ w2 (2^32 - 1)`. Two corners exist only because cy enters the chain: with cy = 1 and
lo0 == hi32(hi') the low word borrows because of the carry alone, and with lo1 == 0 on top the 64-bit borrow (the repair branch) is
caused by the carry alone."""
import collections
import itertools

import numpy as np

import rare_paths as R

P, M64, EPS = R.P, R.M64, R.EPS
Chain = collections.namedtuple("Chain", "cy low_borrow borrow wrap corner lazy")
CLASSES = tuple((cy, lb, b, w) for cy in (0, 1) for lb, b in ((0, 0), (1, 0), (1, 1)) for w in (0, 1))
CORNERS = ("carry_alone_64", "carry_alone_low")

# the edge list of tests/test_gpu_parity.py::test_field_mul_every_carry_and_borrow_corner
EDGE = [0, 1, 2, 3, P - 1, P - 2, P, P + 1, M64, M64 - 1, 0xFFFFFFFF, 0x100000000, 0x100000001, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001,
        1 << 63, (1 << 63) + 1, 0x7FFFFFFF80000000, 0x8000000080000000, 0xFFFFFFFFFFFF0000, 1 << 48, 3 << 48, 1 << 32, 1 << 33]
HALVES = [0, 1, 2, 3, (1 << 32) - 1, (1 << 32) - 2, (1 << 32) - 3, 1 << 31, (1 << 31) + 1, (1 << 31) - 1, 1 << 16, (1 << 16) + 1,
          0xFFFF0000, 0x0000FFFF, 0x80000001, 0x7FFFFFFE]


def chain(a, b, c=None):
    """gl::mul_lazy(a, b) (c is None) or gl::mul_add_lazy(a, b, c), instruction by instruction, any u64 operands. Asserts the four
    bounds of gl.h and the congruence; returns the class, the corner (or None) and the lazy result."""
    a, b = int(a), int(b)
    a0, a1, b0, b1 = a & EPS, a >> 32, b & EPS, b >> 32
    p00 = a0 * b0
    p01 = a0 * b1 + (p00 >> 32)
    assert p01 >> 64 == 0
    r = a1 * b0 + p01                        # third multiply-add: 64 bits and a carry-out
    cy, r = r >> 64, r & M64
    assert cy in (0, 1)
    lo = (p00 & EPS) | ((r & EPS) << 32)
    hi = a1 * b1 + (r >> 32)                 # hi': the addend is {hi32(r), 0}
    assert hi <= (1 << 64) - (1 << 32), "(1) hi' carries"
    total = a * b
    if c is not None:
        c = int(c)
        lo += c
        hi += lo >> 64
        lo &= M64
        assert hi >> 64 == 0, "(2) hi' + 1 carries"
        total += c
    assert lo + ((hi + (cy << 32)) << 64) == total
    w2, w3 = hi & EPS, hi >> 32
    assert w3 + cy <= EPS, "(2) hi32(hi') + cy leaves 32 bits"
    lo0, lo1 = lo & EPS, lo >> 32
    d = lo0 - w3 - cy                        # v_subb_co_u32, carry-in = cy
    low_borrow, tl = int(d < 0), d & EPS
    d = lo1 - low_borrow                     # v_subbrev_co_u32
    borrow, th = int(d < 0), d & EPS
    assert borrow == (lo < w3 + cy), "the repair is taken for other operands than lo < w3"
    t0 = tl | (th << 32)
    if borrow:
        assert t0 >= EPS, "(3) the repaired t0 underflows"
        t0 -= EPS
    s = t0 + w2 * EPS                        # fold_top
    wrap = s >> 64
    assert wrap in (0, 1)
    if wrap:
        s = (s & M64) + EPS
        assert s >> 64 == 0, "(4) the fold wraps twice"
    assert s % P == total % P
    corner = None
    if cy and lo0 == w3:
        corner = CORNERS[0] if lo1 == 0 else CORNERS[1]
        assert low_borrow and borrow == (lo1 == 0)
    return Chain(cy, low_borrow, borrow, wrap, corner, s)


def half_operands():
    """all 16^4 (a, b) whose 32-bit halves come from HALVES"""
    for a1, a0, b1, b0 in itertools.product(HALVES, repeat=4):
        yield (a1 << 32) | a0, (b1 << 32) | b0


_WITNESSES = None
PER_KEY = 16


def witnesses():
    """class or corner -> up to PER_KEY operand pairs of that class, from the 16^4 set; computed once"""
    global _WITNESSES
    if _WITNESSES is None:
        w = {k: [] for k in CLASSES + CORNERS}
        count = collections.Counter()
        for a, b in half_operands():
            ch = chain(a, b)
            for key in (ch[:4], ch.corner):
                if key is not None:
                    count[key] += 1
                    if len(w[key]) < PER_KEY:
                        w[key].append((a, b))
        _WITNESSES = (w, count)
    return _WITNESSES


def witness_array(n=1024, seed=5):
    """(A, B, masks): for every class and corner and every lane pattern of rare_paths.patterns one block of n operand pairs, random
    pairs with that key's witnesses planted under the pattern; masks: [(key, pattern, offset, mask)]"""
    w, _ = witnesses()
    rng = np.random.default_rng(seed)
    A, B, masks = [], [], []
    for key in CLASSES + CORNERS:
        assert w[key], "no witness of %r" % (key,)
        for name, mask in R.patterns(n).items():
            a = rng.integers(0, 1 << 64, n, dtype=np.uint64)
            b = rng.integers(0, 1 << 64, n, dtype=np.uint64)
            for cnt, i in enumerate(np.nonzero(mask)[0]):
                a[i], b[i] = w[key][cnt % len(w[key])]
            masks.append((key, name, n * len(A), mask))
            A.append(a)
            B.append(b)
    return np.concatenate(A), np.concatenate(B), masks


# ---- Poseidon: first S-box operands that are (cy = 1, repaired) ----------------------------------------------------------------
MAX_REJECTIONS = 64


def sbox_carry_borrow_element(i, rng):
    """canonical e with x = e + rc(i) exactly (no wrap), x lazy, whose first squaring x x of the S-box has cy = 1 and takes the
    repair: x = 2^64 - j or 2^63 - j, so the low 64 bits of x^2 are j^2 < 2^32 under a w3 of 2^32 - 1 / 2^30 - 1, and both cross
    terms are large. (rare_paths.sbox_borrow_element's x = k << 32 has a zero low word: no cross terms, cy = 0 always.) Rejection on
    the class, at most MAX_REJECTIONS draws."""
    c = R.RC[i]
    for _ in range(MAX_REJECTIONS + 1):
        j = int(rng.integers(1, 1 << 16))
        x = ((1 << 64) if rng.integers(0, 2) else (1 << 63)) - j
        e = x - c
        if 0 <= e < P:
            ch = chain(x, x)
            if ch.cy and ch.borrow:
                return e, x
    raise AssertionError("more than %d rejections for constant %d" % (MAX_REJECTIONS, i))


def poseidon_carry_borrow_states(mask, seed):
    """rare_paths.poseidon_borrow_states with (cy = 1, repaired) first squarings in all twelve S-boxes of round 0 under the mask"""
    st, _ = R.poseidon_borrow_states(np.zeros(mask.size, bool), seed)
    rng = np.random.default_rng(seed + 1)
    wit = []
    for r in np.nonzero(mask)[0]:
        for i in range(R.W):
            st[r, i], x = sbox_carry_borrow_element(i, rng)
            wit.append((x, x))
    return st, wit


def hash_carry_borrow_rows(length, mask, seed):
    """(n, length) inputs of hash_no_pad: under the mask every absorbed element (position c meets rc(c % 8), rare_paths.leaf_columns)
    makes the first squaring of its S-box a (cy = 1, repaired) product"""
    cols, _ = R.leaf_columns(length, np.zeros(mask.size, bool), seed)
    rng = np.random.default_rng(seed + 1)
    wit = []
    for j in np.nonzero(mask)[0]:
        for c in range(length):
            cols[c, j], x = sbox_carry_borrow_element(c % 8, rng)
            wit.append((x, x))
    return np.ascontiguousarray(cols.T), wit
