"""Operands for the paired product of csrc/gl.h (`mul_lazy2`: two product chains issued alternately, their borrow masks ORed and tested
once, both repaired behind that one branch). What can go wrong in a pair and not in a single product is the coupling: chain A's
carries read in chain B, the repair of one chain applied to the other, a mask taken for the wrong lanes. So the array holds every
class of tests/product_chain.py in slot A against every class in slot B, under every lane pattern. Pure Python, no GPU."""
import numpy as np

import product_chain as C
import rare_paths as R

P, M64 = C.P, C.M64
KEYS = C.CLASSES + C.CORNERS
N = 1024   # elements per (class pair, lane pattern) block


def key_of(ch):
    """the keys (class, and corner if any) a chain belongs to"""
    return (ch[:4],) + ((ch.corner,) if ch.corner else ())


def repairs(key):
    """does a product of this class or corner take the 64-bit borrow repair?"""
    return bool(key[2]) if key in C.CLASSES else key == C.CORNERS[0]


_PAIRS = None


def pair_array(seed=9):
    """(A, B, C_, D, blocks): slot A computes A * B, slot B computes C_ * D in the same lane. For every (key_a, key_b) in KEYS x KEYS
    and every lane pattern one block of N lanes: random operands, with witnesses of key_a planted in slot A and of key_b in slot B under
    the pattern. blocks: [(key_a, key_b, pattern, offset, mask)]. Computed once."""
    global _PAIRS
    if _PAIRS is None:
        w, _ = C.witnesses()
        rng = np.random.default_rng(seed)
        pats = R.patterns(N)
        cols = [[], [], [], []]
        blocks = []
        off = 0
        for ka in KEYS:
            for kb in KEYS:
                for name in R.PATTERNS:
                    mask = pats[name]
                    v = [rng.integers(0, 1 << 64, N, dtype=np.uint64) for _ in range(4)]
                    for cnt, i in enumerate(np.nonzero(mask)[0]):
                        v[0][i], v[1][i] = w[ka][cnt % len(w[ka])]
                        v[2][i], v[3][i] = w[kb][(cnt + 5) % len(w[kb])]
                    for c, x in zip(cols, v):
                        c.append(x)
                    blocks.append((ka, kb, name, off, mask))
                    off += N
        _PAIRS = tuple(np.concatenate(c) for c in cols) + (blocks,)
    return _PAIRS


_WANT = None


def pair_products():
    """(a b mod p, c d mod p) of `pair_array` with Python integers; computed once"""
    global _WANT
    if _WANT is None:
        A, B, C_, D, _ = pair_array()
        _WANT = (np.array([x * y % P for x, y in zip(A.tolist(), B.tolist())], dtype=np.uint64),
                 np.array([x * y % P for x, y in zip(C_.tolist(), D.tolist())], dtype=np.uint64))
    return _WANT


# ---- Poseidon: the two partners of a first-round S-box pair ------------------------------------------------------------------------
COMBOS = ((1, 0), (0, 1), (1, 1))   # (first partner's squaring repairs, second partner's)
PAIR_POSITIONS = R.W // 2           # permute_until pairs words (0, 1) ... (10, 11) of a full round


def add_const_lazy(a, c):
    """poseidon.h add_const_lazy"""
    s = a + c
    if s >> 64:
        s = (s & M64) + C.EPS
    return s


def poseidon_pair_states(n=256, seed=70):
    """(n, 12) states and [(row, position, combo)]: row r has one first-round pair (words 2 q, 2 q + 1) whose partners' first squarings
    are (cy = 1, repaired) as COMBOS[r % 3] says, q = (r // 3) % 6; every other word is random. The planted words come from
    product_chain.poseidon_carry_borrow_states."""
    planted, _ = C.poseidon_carry_borrow_states(np.ones(n, bool), seed)
    st, _ = C.poseidon_carry_borrow_states(np.zeros(n, bool), seed + 7)
    what = []
    for r in range(n):
        combo, q = COMBOS[r % 3], (r // 3) % PAIR_POSITIONS
        for h in range(2):
            if combo[h]:
                st[r, 2 * q + h] = planted[r, 2 * q + h]
        what.append((r, q, combo))
    return st, what


def first_squaring(st, r, i):
    """the chain of the first product x x of word i's S-box in round 0"""
    x = add_const_lazy(int(st[r, i]), R.RC[i])
    return C.chain(x, x)
