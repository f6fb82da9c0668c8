"""Seeded constraint systems for tests/test_gpu_r1cs.py and tools/bench_r1cs.py, with their evaluation in Python integers.

A system is a dict: n (constraints), n_wires, coeffs (list of ints: the table), mats (three (row_ptr uint64, col uint32, coeff uint32)
numpy triples: A, B, C in CSR), w (list of ints: the witness, w[0] = 1). Nothing here touches the GPU or the library."""
import numpy as np

import oracle_lib as O

R = O.bls_constants()[1]
LONG_ROW_THRESHOLD = 128      # city-rollup_amd/csrc/r1cs.h: a row of more terms takes a workgroup


def limbs4(vals):
    """ints -> (len, 4) uint64 little-endian limbs"""
    return np.array([[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def from_limbs4(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192 for x in a]


def coefficient_table(rng, n_random=20):
    """every kind of coefficient the kernels tell apart, the edges of each class included"""
    special = [0, 1, R - 1, 2, R - 2, 12345, (1 << 28) - 1, 1 << 28, R - (1 << 28) + 1, R - (1 << 28), (1 << 64) - 1, 1 << 64, R - 12345]
    return special + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n_random)]


def witness_values(rng, n_wires):
    w = [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n_wires)]
    for i, v in zip(range(n_wires), [1, 0, 1, R - 1, 2, R - 2]):
        w[i] = v
    for i in range(6, n_wires, 7):   # the special values again, spread over the wires
        w[i] = (0, 1, R - 1)[(i // 7) % 3]
    return w


def eval_row(sys_, m, j):
    row_ptr, col, coeff = sys_["mats"][m]
    lo, hi = int(row_ptr[j]), int(row_ptr[j + 1])
    w, cs = sys_["w"], sys_["coeffs"]
    return sum(cs[k] * w[c] for c, k in zip(col[lo:hi].tolist(), coeff[lo:hi].tolist())) % R


def eval_all(sys_):
    """three lists of n values"""
    return [[eval_row(sys_, m, j) for j in range(sys_["n"])] for m in range(3)]


def violated_rows(sys_):
    a, b, c = eval_all(sys_)
    return [j for j in range(sys_["n"]) if a[j] * b[j] % R != c[j]]


def row_lengths(sys_, m):
    rp = sys_["mats"][m][0].astype(np.int64)
    return rp[1:] - rp[:-1]


def kept_lengths(sys_, m):
    """terms per row that the library keeps: a term whose coefficient is 0 is dropped at create"""
    row_ptr, _, coeff = sys_["mats"][m]
    kept = np.array([c != 0 for c in sys_["coeffs"]])[coeff].astype(np.int64)
    cum = np.concatenate([np.zeros(1, np.int64), np.cumsum(kept)])
    return cum[row_ptr[1:].astype(np.int64)] - cum[row_ptr[:-1].astype(np.int64)]


def long_rows(sys_):
    """the rows that take a workgroup: more than the threshold of kept terms"""
    return [(m, int(j)) for m in range(3) for j in np.nonzero(kept_lengths(sys_, m) > LONG_ROW_THRESHOLD)[0]]


def random_system(n, seed, with_long=True, n_wires=None):
    """An arbitrary (unsatisfied) system for evaluation parity. Its 3 n rows are given, in this order of priority and as far as
    they go, the shapes the kernels must get right: a row of 100 000 terms, one of 5 000 (both with repeated wires: there are fewer
    wires than terms), an empty row, a one-term row, a row that names one wire twice, a row of exactly the long-row threshold
    and one of a term more, a row of every coefficient of the table on wire 0; the rest draw their length from a skewed
    distribution (10 % empty, 25 % one term, most below 8, a few up to 100). 35 % of all terms are on wire 0; 40 % of the
    coefficients are 1, 20 % are -1, 15 % one-limb, the rest anything of the table. n = 1 therefore has the two long rows and the
    empty row, n = 2 adds the one-term, repeated-wire and threshold rows, n >= 3 has everything."""
    rng = np.random.default_rng(seed)
    n_wires = n_wires or max(24, min(n, 4096))
    coeffs = coefficient_table(rng)
    w = witness_values(rng, n_wires)
    n_rows = 3 * n
    u = rng.random(n_rows)
    lens = np.where(u < 0.10, 0, np.where(u < 0.35, 1, np.where(u < 0.97, rng.integers(2, 8, n_rows), rng.integers(8, 101, n_rows)))).astype(np.int64)
    forced = ([100_000, 5_000] if with_long else []) + [0, 1, 2, LONG_ROW_THRESHOLD, LONG_ROW_THRESHOLD + (1 if with_long else 0), len(coeffs)]
    # spread over the matrices and over the rows: slot s -> matrix s % 3, row (s // 3) * stride
    stride = max(1, n // ((len(forced) + 2) // 3 + 1))
    slots = {}
    for s, ln in enumerate(forced):
        m, j = s % 3, (s // 3) * stride
        if j < n:
            slots[s] = (m, j)
            lens[m * n + j] = ln
    total = int(lens.sum())
    col = rng.integers(0, n_wires, total, dtype=np.int64)
    col[rng.random(total) < 0.35] = 0
    one_limb = [i for i, c in enumerate(coeffs) if 2 <= c < (1 << 28) or 2 <= R - c < (1 << 28)]
    v = rng.random(total)
    coeff = rng.integers(0, len(coeffs), total, dtype=np.int64)
    coeff[v < 0.40] = coeffs.index(1)
    coeff[(v >= 0.40) & (v < 0.60)] = coeffs.index(R - 1)
    pick = (v >= 0.60) & (v < 0.75)
    coeff[pick] = np.array(one_limb)[rng.integers(0, len(one_limb), int(pick.sum()))]
    start = np.concatenate([[0], np.cumsum(lens)])
    for s, (m, j) in slots.items():
        lo = int(start[m * n + j])
        if forced[s] == 2:                       # one wire twice
            col[lo + 1] = col[lo]
        if forced[s] == len(coeffs):             # every coefficient on the constant wire
            col[lo:lo + len(coeffs)] = 0
            coeff[lo:lo + len(coeffs)] = np.arange(len(coeffs))
    mats = []
    for m in range(3):
        lo, hi = int(start[m * n]), int(start[(m + 1) * n])
        mats.append(((start[m * n:(m + 1) * n + 1] - start[m * n]).astype(np.uint64), col[lo:hi].astype(np.uint32), coeff[lo:hi].astype(np.uint32)))
    return {"n": n, "n_wires": n_wires, "coeffs": coeffs, "mats": mats, "w": w}


def _offsets(lens):
    """position of every term inside its row, rows concatenated"""
    lens = lens.astype(np.int64)
    return np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)


def satisfied_system(n, seed, n_inputs=None, long_lengths=(5_000, 100_000, 300), linear_share=0.4):
    """A satisfied system of n >= 8 constraints with the witness that satisfies it. Three kinds of constraint:
      linear   A = a combination, B = wire 0, C = the same combination, its terms reversed        (no new wire)
      zero     A empty, B a combination, C empty                                                    (5 %)
      product  A, B = combinations, C = k * (a new wire), the wire solved for                      (one new wire)
    Combinations have 1 to 6 terms over the wires that exist so far (35 % wire 0), coefficients as in random_system. The rows
    n/2, n/3 and 2n/3 are long: A of n/2 and B of n/3 (product constraints) and both A and C of 2n/3 (linear). The last
    constraint is a product, so its C row is the only user of the last wire. Everything but the solving of the product wires
    (one pass of Python integers over the product constraints) is numpy."""
    assert n >= 8
    rng = np.random.default_rng(seed)
    coeffs = coefficient_table(rng)
    nonzero = np.array([k for k, c in enumerate(coeffs) if c])
    inv = {int(k): pow(coeffs[k], -1, R) for k in nonzero}
    one, minus_one = coeffs.index(1), coeffs.index(R - 1)
    small_ids = np.array([i for i, c in enumerate(coeffs) if 2 <= c < (1 << 28) or 2 <= R - c < (1 << 28)])
    n_inputs = n_inputs or max(16, min(n // 8, 1 << 16))
    w = witness_values(rng, 1 + n_inputs)
    u = rng.random(n)
    kind = np.where(u < linear_share, 0, np.where(u < linear_share + 0.05, 1, 2))
    kind[n - 1] = 2
    la, lb = rng.integers(1, 7, n), rng.integers(1, 7, n)
    kind[n // 2], la[n // 2] = 2, long_lengths[0]
    kind[n // 3], lb[n // 3] = 2, long_lengths[1]
    kind[(2 * n) // 3], la[(2 * n) // 3] = 0, long_lengths[2]
    product = kind == 2
    avail = 1 + n_inputs + np.cumsum(product) - product          # wires that exist when row j is written
    len_a = np.where(kind == 1, 0, la)
    len_b = np.where(kind == 0, 1, lb)
    len_c = np.where(kind == 0, la, np.where(kind == 1, 0, 1))

    def combination(lens, fixed_one):
        """cols, coefficient indices of the rows concatenated; fixed_one: rows that are just 1 * wire 0"""
        total = int(lens.sum())
        col = (rng.random(total) * np.repeat(avail, lens)).astype(np.int64)
        col[rng.random(total) < 0.35] = 0
        v = rng.random(total)
        k = rng.integers(0, len(coeffs), total)
        k[v < 0.40] = one
        k[(v >= 0.40) & (v < 0.60)] = minus_one
        pick = (v >= 0.60) & (v < 0.75)
        k[pick] = small_ids[rng.integers(0, len(small_ids), int(pick.sum()))]
        fixed = np.repeat(fixed_one, lens)
        col[fixed], k[fixed] = 0, one
        return col, k

    col_a, k_a = combination(len_a, np.zeros(n, bool))
    col_b, k_b = combination(len_b, kind == 0)
    ptr = lambda lens: np.concatenate([np.zeros(1, np.int64), np.cumsum(lens.astype(np.int64))])
    ptr_a, ptr_b, ptr_c = ptr(len_a), ptr(len_b), ptr(len_c)
    # C: a linear row is its A row backwards; a product row is k * the new wire
    src = np.repeat(ptr_a[:-1] + len_a - 1, len_c) - _offsets(len_c)      # valid where the row is linear
    lin = np.repeat(kind == 0, len_c)
    col_c, k_c = np.empty(int(len_c.sum()), np.int64), np.empty(int(len_c.sum()), np.int64)
    col_c[lin], k_c[lin] = col_a[src[lin]], k_a[src[lin]]
    k_new = nonzero[rng.integers(0, len(nonzero), int(product.sum()))]
    col_c[~lin], k_c[~lin] = avail[product], k_new
    # the product wires, in order
    ca, cb = col_a.tolist(), col_b.tolist()
    va, vb = [coeffs[k] for k in k_a.tolist()], [coeffs[k] for k in k_b.tolist()]
    pa, pb = ptr_a.tolist(), ptr_b.tolist()
    for j, k in zip(np.nonzero(product)[0].tolist(), k_new.tolist()):
        a = sum(c * w[i] for i, c in zip(ca[pa[j]:pa[j + 1]], va[pa[j]:pa[j + 1]])) % R
        b = sum(c * w[i] for i, c in zip(cb[pb[j]:pb[j + 1]], vb[pb[j]:pb[j + 1]])) % R
        w.append(a * b % R * inv[k] % R)
    mats = [(p.astype(np.uint64), c.astype(np.uint32), k.astype(np.uint32)) for p, c, k in ((ptr_a, col_a, k_a), (ptr_b, col_b, k_b), (ptr_c, col_c, k_c))]
    return {"n": n, "n_wires": len(w), "coeffs": coeffs, "mats": mats, "w": w}


def from_dict_rows(A, B, C, w):
    """rows given as {wire: coefficient} dicts (the recipe of tests/test_gpu_groth16.py) -> a system: the coefficient table is the
    distinct coefficients in order of first use, as a circuit compiler builds it"""
    table, index = [], {}
    mats = []
    for M in (A, B, C):
        row_ptr, col, coeff = [0], [], []
        for row in M:
            for i, c in row.items():
                if c not in index:
                    index[c] = len(table)
                    table.append(c)
                col.append(i)
                coeff.append(index[c])
            row_ptr.append(len(col))
        mats.append((np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(coeff, np.uint32)))
    return {"n": len(A), "n_wires": len(w), "coeffs": table, "mats": mats, "w": list(w)}


def groth16_case(log_n, n_pub, n_in):
    """The setup of tests/test_gpu_groth16.py::test_groth16_proof_matches_the_trapdoor, restated: a random satisfied R1CS (wire 0 =
    1, public inputs, private inputs, one product wire per constraint), its QAP at a known tau, the logarithms of the proving
    key's points and of the expected proof elements. Returns a dict; the points themselves are made by the test (they need the
    oracle's curve arithmetic and the device)."""
    r = R
    rng = np.random.default_rng(50 + log_n)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % (r - 1) + 1
    n = 1 << log_n
    w = [1] + [rnd() for _ in range(n_pub - 1 + n_in)]
    A, B, C = [], [], []
    for j in range(n):
        avail = len(w)
        ra = {int(i): rnd() for i in rng.choice(avail, size=min(3, avail), replace=False)}
        rb = {int(i): rnd() for i in rng.choice(avail, size=min(2, avail), replace=False)}
        out = sum(c * w[i] for i, c in ra.items()) % r * (sum(c * w[i] for i, c in rb.items()) % r) % r
        w.append(out)
        A.append(ra); B.append(rb); C.append({avail: 1})
    m = len(w)
    dot = lambda row: sum(c * w[i] for i, c in row.items()) % r
    a_ev, b_ev, c_ev = [dot(x) for x in A], [dot(x) for x in B], [dot(x) for x in C]
    assert all(x * y % r == z for x, y, z in zip(a_ev, b_ev, c_ev))
    tau, alpha, beta, delta = rnd(), rnd(), rnd(), rnd()
    omega = pow(7, (r - 1) >> log_n, r)
    zt = (pow(tau, n, r) - 1) % r
    L = [zt * pow(n, -1, r) % r * pow(omega, j, r) % r * pow((tau - pow(omega, j, r)) % r, -1, r) % r for j in range(n)]
    col = lambda M, i: sum(M[j].get(i, 0) * L[j] for j in range(n)) % r
    u, v, ww = [col(A, i) for i in range(m)], [col(B, i) for i in range(m)], [col(C, i) for i in range(m)]
    dinv = pow(delta, -1, r)
    k_log = [(beta * u[i] + alpha * v[i] + ww[i]) * dinv % r for i in range(n_pub, m)]
    z_log = [pow(tau, j, r) * zt % r * dinv % r for j in range(n - 1)]
    interp = lambda ev: sum(e * l for e, l in zip(ev, L)) % r
    h_tau = (interp(a_ev) * interp(b_ev) - interp(c_ev)) * pow(zt, -1, r) % r
    rr, ss = rnd(), rnd()
    a_log = (alpha + sum(x * y for x, y in zip(w, u)) + rr * delta) % r
    b_log = (beta + sum(x * y for x, y in zip(w, v)) + ss * delta) % r
    c_log = (sum(x * y for x, y in zip(w[n_pub:], k_log)) + h_tau * zt * dinv + ss * a_log + rr * b_log - rr * ss * delta) % r
    pub = sum(w[i] * (beta * u[i] + alpha * v[i] + ww[i]) for i in range(n_pub)) % r
    assert a_log * b_log % r == (alpha * beta + pub + c_log * delta) % r
    return {"system": from_dict_rows(A, B, C, w), "evals": (a_ev, b_ev, c_ev), "u": u, "v": v, "k_log": k_log, "z_log": z_log,
            "alpha": alpha, "beta": beta, "delta": delta, "r": rr, "s": ss, "a_log": a_log, "b_log": b_log, "c_log": c_log,
            "n_pub": n_pub, "log_n": log_n}
